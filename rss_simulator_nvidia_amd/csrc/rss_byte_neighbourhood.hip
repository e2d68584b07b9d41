// rss_byte_neighbourhood.hip -- a key's byte neighbourhood (key search's wider local step): the
// per-queue counts -- or, with a weight per tuple, loads -- of the same device-resident tuples
// under every key that differs from one key in ONE BYTE, all 256 values of each of the 16 (IPv6:
// 40) bytes a hash reads, in one launch (rss_key_byte_neighbourhood_device, ..6_device,
// .._weighted_device).  No test hooks: compiled once for both libraries.
//
// Identity.  Toeplitz is linear in the key (rss_neighbourhood.hip): with delta_j(x) = (R >> j) &
// 0xFFFFFFFF the change that flipping key bit j makes to the hash of tuple x, replacing byte B by
// v changes the hash by the XOR of delta_{8B+k}(x) over the set bits 0x80 >> k of d = v ^ key[B].
// The eight deltas of a byte are eight consecutive 32-bit windows of one 64-bit span of R, the
// span at key bit 8B: word = B >> 2 and s0 = 8B & 31 in {0, 8, 16, 24}, so s0 + k <= 31 always.
// The kernel works in d-space -- neighbour d of byte B -- and only the output row is translated
// to v = d ^ key[B]; d = 0 is the key itself.
//
// Work split.  blockIdx.y = (byte, chunk of `ng` consecutive d): d0 = chunk * ng are the chunk's
// high bits, workgroup-uniform, and their deltas go into the base hash once per tuple (an AND
// with a scalar mask and a XOR each).  blockIdx.x is a grid-stride share of the tuples.  ng is a
// power of two <= 32 picked by the bin budget, so a byte is 8 .. 256 chunks.
// Gray walk.  The chunk's low log2(ng) bits are visited in Gray order: step k serves d0 + g,
// g = k ^ (k >> 1), and differs from step k - 1 in bit ctz(k) alone, so it costs ONE XOR with a
// delta that is a compile-time pick among at most five registers -- no shift per neighbour
// (the single-bit kernel pays a v_alignbit and a XOR), and no dependence on anything but the
// previous hash.  Then the bucket / queue step and one LDS add into neighbour g's bin, whose
// offset is an immediate: the bins keep the single-bit kernel's [queue][neighbour][column]
// layout (32 lane columns, one per bank; QM_FAST8's row offset from two 24-bit multiplies).
// With ng at run time (shared bins, global atomics) the same walk runs as a loop: ctz(k) is
// scalar and the delta comes from a select chain over the registers (indexing them would put
// them in scratch).
//
// Bins and tiers are the single-bit entries': the same LDS budget beside the same tables, so
//     IPv4 (161152 B)    ng (private bins)   32    16    8     4     2     1
//                        queues up to        39    78    157   314   629   1259
//                        shared [queue][neighbour]: ng 16 to 2518, 8 to 5036, 4 to 10072,
//                        2 to 20144, 1 to 40288; global atomics past 40288
//     IPv6 (155776 B)    private             38    76    152   304   608   1217
//                        shared: 16 to 2434, 8 to 4868, 4 to 9736, 2 to 19472, 1 to 38944
//     weighted (u64)     private             19    39    78    157   314   629
//                        shared: 16 to 1259, 8 to 2518, 4 to 5036, 2 to 10072, 1 to 20144
// Weighted bins are u64 and every add one ds_add_u64 of the weight (exact for any u32 weights,
// rss_keysearch_weighted.hip).
//
// Flush.  One lane per (queue, neighbour) sums its 32 columns (start column rotated by the row)
// and adds a non-zero sum to row 256 * (B - first_byte) + ((d0 + g) ^ key[B]) with one global
// 64-bit atomic.  The output is cleared by rss_zero_counts_kernel in the same call.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <algorithm>
#include <type_traits>

#include "rss_engine.h"
#include "rss_kernel_common.h"
#include "rss_keysearch_tables.h"

namespace {

// what the byte kernels need beyond LaunchParams: the key's bytes, four per word (byte 4k in
// the top of word k), for the row translation, and the first byte served
struct ByteArgs {
    uint32_t first_byte;
    uint32_t key_words[RSS_KEY6_BYTES / 4];
};

using ByteKernelFn = void (*)(const LaunchParams, const ByteArgs, const uint32_t*);

template <int kWords, bool kWeighted, int kNG, bool kHPow2, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_key_byte_neighbourhood_kernel(
    const LaunchParams p, const ByteArgs a, const uint32_t* __restrict__ weights) {
    using Bin = std::conditional_t<kWeighted, u64, uint32_t>;
    __shared__ uint32_t lut[kNbrLutDwords<kWords>];
    extern __shared__ u64 byte_bins[];
    Bin* bins = reinterpret_cast<Bin*>(byte_bins);
    const uint32_t tid = threadIdx.x;
    const uint32_t ng = kNG ? (uint32_t)kNG : p.nkeys;
    const uint32_t lg = 31 - __clz(ng);                // d bits walked per workgroup
    const uint32_t bi = blockIdx.y >> (8 - lg);        // byte, from first_byte
    const uint32_t d0 = (blockIdx.y << lg) & 0xFFu;    // the chunk's high bits
    const uint32_t B = a.first_byte + bi;
    const uint32_t keyb = (a.key_words[B >> 2] >> (24 - 8 * (B & 3u))) & 0xFFu;
    const uint32_t word = B >> 2, s0 = (8 * B) & 31u;
    if constexpr (kWords == 3) build_small_lut(lut, p.window, tid);
    else build_small_lut6(lut, p.window, tid);
    const uint32_t nrows = p.Q * ng;  // e = q * ng + g
    const uint32_t nbins =
        kHist == HIST_PRIVATE ? nrows * kBinCols : (kHist == HIST_SHARED ? nrows : 0u);
    for (uint32_t e = tid; e < nbins; e += kBlock) bins[e] = 0;
    __syncthreads();

    // d's bit b (0 = LSB) is key bit 8B + 7 - b; the masks of the chunk's high bits are scalar
    uint32_t high[8];
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) high[b] = 0u - ((d0 >> b) & 1u);
    char* bins_colb = reinterpret_cast<char*>(bins + (tid & (kBinCols - 1)));
    constexpr uint32_t kRowBytes = kNG * kBinCols * sizeof(Bin);  // private bins: one queue's row
    // QM_FAST8 (H <= 256) folded into the row's byte offset as in the single-bit kernels:
    // q * row = b * row - d * (Q * row), d = floor(b / Q) -- Q * row <= 161152 and b * row < 2^21
    // fit the 24-bit multiplies
    const int neg_q_row = -(int)(p.Q * kRowBytes);
    u64* rows = p.counts + (size_t)256 * bi * p.q_stride;  // value v of this byte at v * q_stride
    auto count = [&](const uint32_t* w, uint32_t weight) {  // one tuple's kWords words
        uint32_t h;
        uint2 span;
        if constexpr (kWords == 3) {
            h = toeplitz_hash_small(lut, w[0], w[1], w[2]);
            span = flip_span(w[0], w[1], w[2], word, s0);
        } else {
            h = toeplitz_hash_small6(lut, w);
            span = flip_span6(w, word, s0);
        }
        constexpr uint32_t kWalk = kNG ? (uint32_t)(31 - __builtin_clz(kNG | 1)) : 5u;
        uint32_t delta[5];  // of the walked bits (ng <= 32): registers, never indexed at run time
#pragma unroll
        for (uint32_t b = 0; b < 5; ++b) delta[b] = alignbit(span.y, span.x, 7 - b);
#pragma unroll
        for (uint32_t b = kNG ? kWalk : 0u; b < 8; ++b)  // run-time ng: low masks are zero
            h ^= alignbit(span.y, span.x, 7 - b) & high[b];
        auto neighbour = [&](uint32_t g) {
            const uint32_t b = bucket_of<kHPow2>(h, p);
            if constexpr (kHist == HIST_PRIVATE) {
                uint32_t row;
                if constexpr (kQMode == QM_FAST8) {
                    const uint32_t d = __umul24(b, p.q_m16) >> 16;
                    row = (uint32_t)__mul24((int)d, neg_q_row) + b * kRowBytes;
                } else {
                    row = queue_of<kQMode>(b, p) * kRowBytes;
                }
                __hip_atomic_fetch_add(reinterpret_cast<Bin*>(bins_colb + row) + g * kBinCols,
                                       (Bin)weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else if constexpr (kHist == HIST_SHARED) {
                __hip_atomic_fetch_add(&bins[queue_of<kQMode>(b, p) * ng + g], (Bin)weight,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                atomicAdd(&rows[(size_t)((d0 + g) ^ keyb) * p.q_stride + queue_of<kQMode>(b, p)],
                          (u64)weight);
            }
        };
        neighbour(0);
        if constexpr (kNG != 0) {
#pragma unroll
            for (uint32_t k = 1; k < (uint32_t)kNG; ++k) {
                h ^= delta[__builtin_ctz(k)];
                neighbour(k ^ (k >> 1));
            }
        } else {
            for (uint32_t k = 1; k < ng; ++k) {
                const uint32_t t = (uint32_t)__builtin_ctz(k);  // uniform
                h ^= t == 0 ? delta[0] : t == 1 ? delta[1] : t == 2 ? delta[2]
                   : t == 3 ? delta[3] : delta[4];
                neighbour(k ^ (k >> 1));
            }
        }
    };
    const uint64_t gtid = (uint64_t)blockIdx.x * kBlock + tid;
    const uint64_t gstride = (uint64_t)gridDim.x * kBlock;
    uint64_t tail_begin = 0;
    const uintptr_t align = (uintptr_t)p.tuples | (kWeighted ? (uintptr_t)weights : 0u);
    if ((align & 15u) == 0) {  // uniform; 16-byte aligned: four tuples (and weights) per lane
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.tuples);
        const uint4* __restrict__ wsrc = reinterpret_cast<const uint4*>(weights);
        const uint64_t ngroups = p.n >> 2;
        for (uint64_t g = gtid; g < ngroups; g += gstride) {  // kWords x 16 B = four tuples
            uint32_t w[4 * kWords];
#pragma unroll
            for (int i = 0; i < kWords; ++i) {
                const uint4 x = src[kWords * g + i];
                w[4 * i + 0] = x.x;
                w[4 * i + 1] = x.y;
                w[4 * i + 2] = x.z;
                w[4 * i + 3] = x.w;
            }
            uint4 wt = make_uint4(1u, 1u, 1u, 1u);
            if constexpr (kWeighted) wt = wsrc[g];
            count(w + 0 * kWords, wt.x);
            count(w + 1 * kWords, wt.y);
            count(w + 2 * kWords, wt.z);
            count(w + 3 * kWords, wt.w);
        }
        tail_begin = ngroups << 2;
    }
    for (uint64_t i = tail_begin + gtid; i < p.n; i += gstride) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(p.tuples) + kWords * i;
        uint32_t w[kWords];
#pragma unroll
        for (int k = 0; k < kWords; ++k) w[k] = t[k];
        uint32_t weight = 1u;
        if constexpr (kWeighted) weight = weights[i];
        count(w, weight);
    }
    if constexpr (kHist != HIST_GLOBAL) {
        __syncthreads();
        for (uint32_t e = tid; e < nrows; e += kBlock) {
            u64 s;
            if constexpr (kHist != HIST_PRIVATE) {
                s = bins[e];
            } else if constexpr (kWeighted) {
                s = row_sum(byte_bins, e);
            } else {
                uint32_t s32 = 0;
                for (uint32_t c = 0; c < kBinCols; ++c)
                    s32 += bins[e * kBinCols + ((c + e) & (kBinCols - 1))];
                s = s32;
            }
            if (s)
                atomicAdd(&rows[(size_t)((d0 + (e & (ng - 1))) ^ keyb) * p.q_stride + (e >> lg)], s);
        }
    }
}

template <int kWords, bool kWeighted, int kNG, bool kHPow2, int kHist>
ByteKernelFn pick_byte_qmode(int qmode) {
    switch (qmode) {
        case QM_MASK:
            return rss_key_byte_neighbourhood_kernel<kWords, kWeighted, kNG, kHPow2, QM_MASK, kHist>;
        case QM_FAST8:
            return rss_key_byte_neighbourhood_kernel<kWords, kWeighted, kNG, kHPow2, QM_FAST8, kHist>;
        case QM_FAST16:
            return rss_key_byte_neighbourhood_kernel<kWords, kWeighted, kNG, kHPow2, QM_FAST16, kHist>;
        default:
            return rss_key_byte_neighbourhood_kernel<kWords, kWeighted, kNG, kHPow2, QM_FAST32, kHist>;
    }
}

template <int kWords, bool kWeighted, int kNG, int kHist>
ByteKernelFn pick_byte_modes(bool h_pow2, int qmode) {
    return h_pow2 ? pick_byte_qmode<kWords, kWeighted, kNG, true, kHist>(qmode)
                  : pick_byte_qmode<kWords, kWeighted, kNG, false, kHist>(qmode);
}

template <int kWords, bool kWeighted>
ByteKernelFn pick_byte(int hist, uint32_t ng, bool h_pow2, int qmode) {
    if (hist == HIST_SHARED) return pick_byte_modes<kWords, kWeighted, 0, HIST_SHARED>(h_pow2, qmode);
    if (hist != HIST_PRIVATE) return pick_byte_modes<kWords, kWeighted, 0, HIST_GLOBAL>(h_pow2, qmode);
    switch (ng) {
        case 32: return pick_byte_modes<kWords, kWeighted, 32, HIST_PRIVATE>(h_pow2, qmode);
        case 16: return pick_byte_modes<kWords, kWeighted, 16, HIST_PRIVATE>(h_pow2, qmode);
        case 8: return pick_byte_modes<kWords, kWeighted, 8, HIST_PRIVATE>(h_pow2, qmode);
        case 4: return pick_byte_modes<kWords, kWeighted, 4, HIST_PRIVATE>(h_pow2, qmode);
        case 2: return pick_byte_modes<kWords, kWeighted, 2, HIST_PRIVATE>(h_pow2, qmode);
        default: return pick_byte_modes<kWords, kWeighted, 1, HIST_PRIVATE>(h_pow2, qmode);
    }
}

// Workgroups along x.  Below one round of workgroups (gy < cu_count) the single-bit rule holds:
// as many x slices as fill the round, none smaller than neighbourhood_grid_x's fixed-cost floor.
// The byte grid usually has more rows than the device has CUs (8 .. 256 chunks per byte, up to
// 10240 rows), and cu_count / gy is then 1: one workgroup walks all n tuples, which keeps its
// fixed cost (clearing and summing a CU's worth of bins) smallest -- right when gy is a multiple
// of cu_count, as 16 bytes x 16 .. 256 chunks are on 256 CUs.  When it is not (40 bytes x 8 = 320
// rows run as two rounds, the second a quarter full), x slices even the rounds out: with one
// workgroup per CU the launch takes ceil(x * gy / cu_count) rounds of n / x tuples, so x in
// 1 .. 8 is the one with the smallest rounds / x (320 rows: x = 4, five full rounds; ties go to
// the smaller x), never below the floor either.
inline unsigned byte_grid_x(size_t n, uint32_t q_eff, unsigned gy, int cu_count) {
    const unsigned floor_x = neighbourhood_grid_x(n, q_eff, 1u, 1 << 30);  // slices of the floor
    if ((int)gy < cu_count) return neighbourhood_grid_x(n, q_eff, gy, cu_count);
    unsigned best = 1;
    uint64_t best_rounds = ((uint64_t)gy + cu_count - 1) / cu_count;
    for (unsigned x = 2; x <= std::min(8u, floor_x); ++x) {
        const uint64_t rounds = ((uint64_t)x * gy + cu_count - 1) / cu_count;
        if (rounds * best < best_rounds * x) {  // rounds / x < best_rounds / best
            best = x;
            best_rounds = rounds;
        }
    }
    return best;
}

// clear, then one launch over nbytes * 256 rows; p holds the key's windows and the tuples
template <int kWords, bool kWeighted>
int launch_byte_rows(LaunchParams& p, const ByteArgs& a, uint32_t nbytes, uint32_t budget,
                     const uint32_t* d_weights, uint32_t htable, uint32_t nqueues,
                     uint64_t* d_counts, hipStream_t stream) {
    int rc = rss::launch_zero_counts(d_counts, (uint64_t)nbytes * 256 * nqueues, stream);
    if (rc || p.n == 0) return rc;
    DeviceInfo info;
    rc = device_info(&info);
    if (rc) return rc;
    p.counts = reinterpret_cast<unsigned long long*>(d_counts);
    p.q_stride = nqueues;  // rows keep the caller's nqueues; queues >= min(H, Q) stay zero
    const uint32_t q_eff = effective_queues(htable, nqueues, nullptr);
    int qmode, hist;
    uint32_t bin_bytes;  // of one neighbour, as u32 bins: setup_modes sizes those, so u64 bins
                         // get half the budget (rss_keysearch_weighted.hip)
    const bool h_pow2 = setup_modes(&p, htable, q_eff, true, &qmode, &hist, &bin_bytes,
                                    kWeighted ? budget / 2 : budget);
    const uint32_t nbr_bytes = (kWeighted ? 2u : 1u) * bin_bytes;
    const uint32_t ng = hist == HIST_GLOBAL ? 32u : neighbours_per_workgroup(nbr_bytes, budget);
    p.nkeys = ng;
    const unsigned gy = nbytes * (256u / ng);  // <= 10240
    const unsigned gx =
        byte_grid_x(p.n, hist == HIST_PRIVATE ? q_eff : q_eff / kBinCols, gy, info.cu_count);
    hipLaunchKernelGGL((pick_byte<kWords, kWeighted>(hist, ng, h_pow2, qmode)), dim3(gx, gy),
                       dim3(kBlock), nbr_bytes * ng, stream, p, a, d_weights);
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

}  // namespace

// ------------------------------------------------------ launchers (rss_engine.h) --
namespace rss {

int launch_byte_neighbourhood(const rss_key* key, uint32_t first_byte, uint32_t nbytes,
                              const rss_tuple4* d_tuples, const uint32_t* d_weights, size_t n,
                              uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                              hipStream_t stream) {
    LaunchParams p;
    memset(&p, 0, sizeof p);
    memcpy(p.window, key->window, sizeof p.window);
    p.tuples = d_tuples;
    p.n = n;
    ByteArgs a;
    memset(&a, 0, sizeof a);
    a.first_byte = first_byte;
    for (int b = 0; b < RSS_KEY_BYTES; ++b) a.key_words[b >> 2] |= (uint32_t)key->bytes[b] << (24 - 8 * (b & 3));
    if (d_weights)
        return launch_byte_rows<3, true>(p, a, nbytes, kNbrBinBytesMax, d_weights, htable, nqueues,
                                         d_counts, stream);
    return launch_byte_rows<3, false>(p, a, nbytes, kNbrBinBytesMax, nullptr, htable, nqueues,
                                      d_counts, stream);
}

int launch_byte_neighbourhood6(const rss_key6* key, uint32_t first_byte, uint32_t nbytes,
                               const rss_tuple6* d_tuples, size_t n, uint32_t htable,
                               uint32_t nqueues, uint64_t* d_counts, hipStream_t stream) {
    LaunchParams p;
    memset(&p, 0, sizeof p);
    // a plain Toeplitz key (checked by the caller): window 32 k is key word k; word 9 = key
    // bits [288, 319) from the last window.  Bit 319 feeds no hash and rss_key6 keeps no bytes:
    // it reads as 0 here, which only swaps the equal rows v and v ^ 1 of byte 39.
    for (int k = 0; k < kWords6; ++k) p.window[k] = key->window[32 * k];
    p.window[kWords6] = key->window[RSS_INPUT6_BITS - 1] << 1;
    p.tuples = reinterpret_cast<const rss_tuple4*>(d_tuples);  // read as dwords / uint4 only
    p.n = n;
    ByteArgs a;
    a.first_byte = first_byte;
    memcpy(a.key_words, p.window, sizeof a.key_words);
    return launch_byte_rows<kWords6, false>(p, a, nbytes, kNbr6BinBytesMax, nullptr, htable,
                                            nqueues, d_counts, stream);
}

}  // namespace rss
