// rss_keysearch_weighted.hip -- key search by traffic load: the search and neighbourhood
// launches with a weight per tuple (packets or bytes of the flow) instead of 1, so that keys
// are ranked by the load they put on each queue and not by the number of flows
// (rss_key_search_weighted_device, rss_key_neighbourhood_weighted_device).  No test hooks:
// compiled once for both libraries.
//
// Hashing is the unweighted kernels' (rss_keysearch_tables.h): the packed small tables for 8 /
// 4 keys per ds_read_b64 (power-of-two H <= 256 / <= 65536), the wide pair tables for any H,
// and for the neighbourhood one base hash on the 4-byte small tables plus a v_alignbit delta
// per neighbour.  What is new is everything after the queue is known.
//
// Bins.  A weight is any u32 and a workgroup may see 2^20 tuples, so a u32 bin could wrap after
// two tuples; the bins are u64 and every add is one ds_add_u64 of {weight, 0} -- exact by
// construction (n < 2^32 tuples x (2^32 - 1) < 2^64), no epochs, no branch.  They keep the
// unweighted layout's 32 lane columns, [queue][key or neighbour][column]: a (queue, key) row is
// 32 x 8 B = 256 B, the LDS's 64 banks exactly once, so the lanes of a half-wave -- 32
// different columns -- sit on 32 different bank pairs whatever their queues and keys are, and a
// ds_add_u64 never conflicts.  16 columns (the same keys per workgroup in the same bytes) would
// put two lanes of every half-wave on one bank pair whenever their rows have the same parity:
// half the rows' adds at half rate.  So the columns stay and each tier's queue bound halves:
//   search, packed tables (154.75 KiB of bins)   8 keys to Q = 77, 4 keys to Q = 154
//   search, pair tables (40 KiB of bins, 2 keys) lane-private to Q = 80, shared [queue] to 2560
//   neighbourhood (161152 B of bins)   ng     32   16   8    4    2    1
//     lane-private, queues up to              19   39   78   157  314  629
//     shared [queue][neighbour], up to        --   1259 2518 5036 10072 20144
// and past the last LDS tier one global 64-bit atomicAdd of the weight per (tuple, key).
// The key's or neighbour's 256-byte offset is the ds_add's immediate and the queue's row a
// multiple of a compile-time size, as in the unweighted kernels.
//
// Input.  The weights are an array of their own (resident tuple buffers are reused as they
// are): with both pointers 16-byte aligned a lane takes four tuples through three dwordx4
// loads and their four weights through a fourth -- 64 B per lane-step instead of 48 -- and the
// n % 4 tail, or any other alignment, goes one tuple and one weight per lane through dword
// loads.  The choice is a uniform branch on the pointers, not a template parameter.
//
// Flush.  Each (queue, key) row's 32 columns are summed as u64 by one lane (the start column
// rotated by the row so that neighbouring lanes read different banks) and a non-zero sum is
// one global 64-bit atomicAdd.  The loads are cleared by rss_zero_counts_kernel in the same
// call, so the entries can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <algorithm>

#include "rss_engine.h"
#include "rss_kernel_common.h"
#include "rss_keysearch_tables.h"

namespace {

using WeightedKernelFn = void (*)(const LaunchParams, const uint32_t*);

__device__ __forceinline__ void lds_add_load(u64* bin, uint32_t weight) {  // ds_add_u64
    __hip_atomic_fetch_add(bin, (u64)weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The grid's walk: `count(w0, w1, w2, weight)` for this lane's share of the tuples.
template <typename Count>
__device__ __forceinline__ void walk_weighted(const LaunchParams& p,
                                              const uint32_t* __restrict__ weights, Count count) {
    const uint64_t gtid = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint64_t gstride = (uint64_t)gridDim.x * kBlock;
    uint64_t tail_begin = 0;
    if ((((uintptr_t)p.tuples | (uintptr_t)weights) & 15u) == 0) {  // uniform
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.tuples);
        const uint4* __restrict__ wsrc = reinterpret_cast<const uint4*>(weights);
        const uint64_t ngroups = p.n >> 2;
        for (uint64_t g = gtid; g < ngroups; g += gstride) {
            const uint4 a = src[3 * g + 0];
            const uint4 b = src[3 * g + 1];
            const uint4 c = src[3 * g + 2];
            const uint4 w = wsrc[g];
            count(a.x, a.y, a.z, w.x);
            count(a.w, b.x, b.y, w.y);
            count(b.z, b.w, c.x, w.z);
            count(c.y, c.z, c.w, w.w);
        }
        tail_begin = ngroups << 2;
    }
    for (uint64_t i = tail_begin + gtid; i < p.n; i += gstride) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(p.tuples) + 3 * i;
        count(t[0], t[1], t[2], weights[i]);
    }
}

// ------------------------------------------------------------ search, packed tables --
// 8 (byte lanes, H <= 256) or 4 (half-word lanes, H <= 65536) keys per workgroup on the 21
// conflict-free ds_read_b64 of the unweighted packed kernel; bins u64 [queue][key][column].
template <int kLaneBits, int kQMode>
__global__ __launch_bounds__(kBlock) void rss_key_search_weighted_packed_kernel(
    const LaunchParams p, const uint32_t* __restrict__ weights) {
    constexpr uint32_t kKeys = 64 / kLaneBits;
    __shared__ uint2 lut[kPairLutBytes / 8];
    extern __shared__ u64 loads[];
    const uint32_t tid = threadIdx.x;
    const uint32_t key0 = kKeys * blockIdx.y;

    // lane k of packed[i] = low kLaneBits of key (key0 + k)'s window i (a key past the end
    // repeats the last key; its loads are discarded)
    uint2* packed = reinterpret_cast<uint2*>(loads);
    if (tid < RSS_INPUT_BITS) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t k = 0; k < kKeys; ++k) {
            const uint32_t key = min(key0 + k, p.nkeys - 1);
            const uint32_t w = p.key_windows[(size_t)RSS_INPUT_BITS * key + tid] &
                               ((1u << kLaneBits) - 1);
            const uint32_t shift = k * kLaneBits;
            if (shift < 32) lo |= w << shift;
            else hi |= w << (shift - 32);
        }
        packed[tid] = make_uint2(lo, hi);
    }
    __syncthreads();
    build_small_pair_lut(lut, [&](int i) { return packed[i]; }, tid);
    __syncthreads();  // packed windows are dead: the region becomes bins
    const uint32_t nrows = p.Q * kKeys;
    for (uint32_t e = tid; e < nrows * kBinCols; e += kBlock) loads[e] = 0;
    __syncthreads();

    char* col = reinterpret_cast<char*>(loads + (tid & (kBinCols - 1)));
    const uint32_t hbits = 31 - __clz(p.H);  // log2(H)
    constexpr uint32_t kRowShift = kLaneBits == 8 ? 11 : 10;  // log2(kKeys * kLoadRowBytes)
    // byte lanes: q * 2^kRowShift = (b << kRowShift) - d * (Q << kRowShift), d = floor(b / Q):
    // two full-rate 24-bit multiplies (Q <= 77 rows of 2 KiB and b < 256 fit 24 bits)
    const int neg_q_row = -(int)(p.Q << kRowShift);
    const uint32_t lane_mask4 = (p.H - 1) * 0x01010101u;
    walk_weighted(p, weights, [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t weight) {
        uint2 x = toeplitz_hash_pair(lut, w0, w1, w2);
        if constexpr (kLaneBits == 8) {
            x.x &= lane_mask4;
            x.y &= lane_mask4;
        }
#pragma unroll
        for (uint32_t k = 0; k < kKeys; ++k) {
            const uint32_t word = (k * kLaneBits) < 32 ? x.x : x.y;
            const uint32_t b = kLaneBits == 8 ? (word >> ((k * 8) & 31)) & 0xFFu
                                              : __builtin_amdgcn_ubfe(word, (k * kLaneBits) & 31, hbits);
            uint32_t row;
            if constexpr (kLaneBits == 8 && kQMode == QM_FAST16) {
                const uint32_t d = __umul24(b, p.q_m16) >> 16;
                row = (uint32_t)__mul24((int)d, neg_q_row) + (b << kRowShift);
            } else {
                row = queue_of<kQMode>(b, p) << kRowShift;
            }
            lds_add_load(reinterpret_cast<u64*>(col + row) + k * kBinCols, weight);
        }
    });
    __syncthreads();
    for (uint32_t e = tid; e < nrows; e += kBlock) {  // e = q * kKeys + k
        const uint32_t q = e / kKeys, k = e % kKeys;
        if (key0 + k >= p.nkeys) continue;
        const u64 s = row_sum(loads, e);
        if (s) atomicAdd(&p.counts[(size_t)(key0 + k) * p.q_stride + q], s);
    }
}

// -------------------------------------------------------------- search, pair tables --
// Any H: keys 2y and 2y + 1 on the nine wide tables (two full hashes per tuple); bins u64
// [key][queue][column] (private), [key][queue] (shared) or none (global atomics).
template <bool kHPow2, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_key_search_weighted_pair_kernel(
    const LaunchParams p, const uint32_t* __restrict__ weights) {
    __shared__ uint2 lut[kWidePairLutBytes / 8];
    extern __shared__ u64 loads[];
    const uint32_t tid = threadIdx.x;
    // an odd last key is paired with itself and its copy neither flushed nor added
    const uint32_t key_a = 2 * blockIdx.y;
    const bool has_b = key_a + 1 < p.nkeys;
    const uint32_t key_b = has_b ? key_a + 1 : key_a;
    build_wide_pair_lut(lut, p.key_windows + (size_t)RSS_INPUT_BITS * key_a,
                        p.key_windows + (size_t)RSS_INPUT_BITS * key_b, tid);
    const uint32_t per_key =
        kHist == HIST_PRIVATE ? p.Q * kBinCols : (kHist == HIST_SHARED ? p.Q : 0u);
    for (uint32_t e = tid; e < 2 * per_key; e += kBlock) loads[e] = 0;
    __syncthreads();

    u64* rows_a = p.counts + (size_t)key_a * p.q_stride;
    u64* rows_b = p.counts + (size_t)key_b * p.q_stride;
    u64* bins_a = loads + (kHist == HIST_PRIVATE ? tid & (kBinCols - 1) : 0u);
    u64* bins_b = bins_a + per_key;
    uint32_t hi = 65536u;
    asm volatile("" : "+v"(hi));
    walk_weighted(p, weights, [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t weight) {
        const uint2 h = toeplitz_hash_wide_pair(lut, w0, w1, w2, hi);
        const uint32_t qa = queue_of<kQMode>(bucket_of<kHPow2>(h.x, p), p);
        const uint32_t qb = queue_of<kQMode>(bucket_of<kHPow2>(h.y, p), p);
        if constexpr (kHist == HIST_PRIVATE) {
            lds_add_load(bins_a + qa * kBinCols, weight);
            lds_add_load(bins_b + qb * kBinCols, weight);
        } else if constexpr (kHist == HIST_SHARED) {
            lds_add_load(bins_a + qa, weight);
            lds_add_load(bins_b + qb, weight);
        } else {
            atomicAdd(&rows_a[qa], (u64)weight);
            if (has_b) atomicAdd(&rows_b[qb], (u64)weight);
        }
    });
    if constexpr (kHist != HIST_GLOBAL) {
        __syncthreads();
        for (uint32_t e = tid; e < (has_b ? 2 : 1) * p.Q; e += kBlock) {  // e = key * Q + q
            const u64 s = kHist == HIST_PRIVATE ? row_sum(loads, e) : loads[e];
            if (s) atomicAdd(e < p.Q ? &rows_a[e] : &rows_b[e - p.Q], s);
        }
    }
}

// -------------------------------------------------------------------- neighbourhood --
// `ng` consecutive neighbours j0 = ng * blockIdx.y .. per workgroup (kNG, or p.nkeys at run
// time for the shared and global tiers): one base hash per tuple on the 4-byte small tables,
// then per neighbour an alignbit of the tuple's flip span, a XOR, the bucket / queue step and
// one 64-bit add.  Bins u64 [queue][neighbour][column] (private) or [queue][neighbour] (shared).
template <int kNG, bool kHPow2, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_key_neighbourhood_weighted_kernel(
    const LaunchParams p, const uint32_t* __restrict__ weights) {
    __shared__ uint32_t lut[kSmallLutDwords];
    extern __shared__ u64 loads[];
    const uint32_t tid = threadIdx.x;
    const uint32_t ng = kNG ? (uint32_t)kNG : p.nkeys;
    const uint32_t j0 = ng * blockIdx.y;
    const uint32_t word = j0 >> 5, s0 = j0 & 31u;
    build_small_lut(lut, p.window, tid);
    const uint32_t nrows = p.Q * ng;  // e = q * ng + k
    const uint32_t nbins =
        kHist == HIST_PRIVATE ? nrows * kBinCols : (kHist == HIST_SHARED ? nrows : 0u);
    for (uint32_t e = tid; e < nbins; e += kBlock) loads[e] = 0;
    __syncthreads();

    char* col = reinterpret_cast<char*>(loads + (tid & (kBinCols - 1)));
    constexpr uint32_t kRowBytes = kNG * kLoadRowBytes;  // private bins: one queue's row
    // QM_FAST8 (H <= 256) folded into the row's byte offset: q * row = b * row - d * (Q * row),
    // d = floor(b / Q) -- Q * row <= 161152 and b * row < 2^21 fit the 24-bit multiplies
    const int neg_q_row = -(int)(p.Q * kRowBytes);
    u64* rows = p.counts + (size_t)j0 * p.q_stride;  // row k at k * q_stride
    walk_weighted(p, weights, [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t weight) {
        const uint32_t h = toeplitz_hash_small(lut, w0, w1, w2);
        const uint2 span = flip_span(w0, w1, w2, word, s0);
        auto neighbour = [&](uint32_t k) {
            const uint32_t b = bucket_of<kHPow2>(h ^ alignbit(span.y, span.x, k), p);
            if constexpr (kHist == HIST_PRIVATE) {
                uint32_t row;
                if constexpr (kQMode == QM_FAST8) {
                    const uint32_t d = __umul24(b, p.q_m16) >> 16;
                    row = (uint32_t)__mul24((int)d, neg_q_row) + b * kRowBytes;
                } else {
                    row = queue_of<kQMode>(b, p) * kRowBytes;
                }
                lds_add_load(reinterpret_cast<u64*>(col + row) + k * kBinCols, weight);
            } else if constexpr (kHist == HIST_SHARED) {
                lds_add_load(&loads[queue_of<kQMode>(b, p) * ng + k], weight);
            } else {
                atomicAdd(&rows[(size_t)k * p.q_stride + queue_of<kQMode>(b, p)], (u64)weight);
            }
        };
        if constexpr (kNG != 0) {
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)kNG; ++k) neighbour(k);
        } else {
            for (uint32_t k = 0; k < ng; ++k) neighbour(k);
        }
    });
    if constexpr (kHist != HIST_GLOBAL) {
        __syncthreads();
        const uint32_t ng_shift = 31 - __clz(ng);
        for (uint32_t e = tid; e < nrows; e += kBlock) {
            const u64 s = kHist == HIST_PRIVATE ? row_sum(loads, e) : loads[e];
            if (s) atomicAdd(&rows[(size_t)(e & (ng - 1)) * p.q_stride + (e >> ng_shift)], s);
        }
    }
}

// ------------------------------------------------------------------- instance picks --
WeightedKernelFn pick_packed(int lane_bits, int qmode) {
    if (lane_bits == 8)
        return qmode == QM_MASK ? rss_key_search_weighted_packed_kernel<8, QM_MASK>
                                : rss_key_search_weighted_packed_kernel<8, QM_FAST16>;
    return qmode == QM_MASK ? rss_key_search_weighted_packed_kernel<16, QM_MASK>
                            : rss_key_search_weighted_packed_kernel<16, QM_FAST16>;
}

template <bool kHPow2, int kQMode>
WeightedKernelFn pick_pair_hist(int hist) {
    switch (hist) {
        case HIST_PRIVATE: return rss_key_search_weighted_pair_kernel<kHPow2, kQMode, HIST_PRIVATE>;
        case HIST_SHARED: return rss_key_search_weighted_pair_kernel<kHPow2, kQMode, HIST_SHARED>;
        default: return rss_key_search_weighted_pair_kernel<kHPow2, kQMode, HIST_GLOBAL>;
    }
}

template <bool kHPow2>
WeightedKernelFn pick_pair(int qmode, int hist) {
    switch (qmode) {
        case QM_MASK: return pick_pair_hist<kHPow2, QM_MASK>(hist);
        case QM_FAST16: return pick_pair_hist<kHPow2, QM_FAST16>(hist);
        default: return pick_pair_hist<kHPow2, QM_FAST32>(hist);
    }
}

template <int kNG, bool kHPow2, int kHist>
WeightedKernelFn pick_nbr_qmode(int qmode) {
    switch (qmode) {
        case QM_MASK: return rss_key_neighbourhood_weighted_kernel<kNG, kHPow2, QM_MASK, kHist>;
        case QM_FAST8: return rss_key_neighbourhood_weighted_kernel<kNG, kHPow2, QM_FAST8, kHist>;
        case QM_FAST16: return rss_key_neighbourhood_weighted_kernel<kNG, kHPow2, QM_FAST16, kHist>;
        default: return rss_key_neighbourhood_weighted_kernel<kNG, kHPow2, QM_FAST32, kHist>;
    }
}

template <int kNG, int kHist>
WeightedKernelFn pick_nbr_modes(bool h_pow2, int qmode) {
    return h_pow2 ? pick_nbr_qmode<kNG, true, kHist>(qmode) : pick_nbr_qmode<kNG, false, kHist>(qmode);
}

WeightedKernelFn pick_nbr(int hist, uint32_t ng, bool h_pow2, int qmode) {
    if (hist == HIST_SHARED) return pick_nbr_modes<0, HIST_SHARED>(h_pow2, qmode);
    if (hist != HIST_PRIVATE) return pick_nbr_modes<0, HIST_GLOBAL>(h_pow2, qmode);
    switch (ng) {
        case 32: return pick_nbr_modes<32, HIST_PRIVATE>(h_pow2, qmode);
        case 16: return pick_nbr_modes<16, HIST_PRIVATE>(h_pow2, qmode);
        case 8: return pick_nbr_modes<8, HIST_PRIVATE>(h_pow2, qmode);
        case 4: return pick_nbr_modes<4, HIST_PRIVATE>(h_pow2, qmode);
        case 2: return pick_nbr_modes<2, HIST_PRIVATE>(h_pow2, qmode);
        default: return pick_nbr_modes<1, HIST_PRIVATE>(h_pow2, qmode);
    }
}

}  // namespace

// ------------------------------------------------------ launchers (rss_engine.h) --
namespace rss {

// Tier table.  setup_modes sizes u32 bins, so it is given half of each budget:
// a tier that holds Q x 32 x 4 B in half the room holds Q x 32 x 8 B in all of it.
int launch_search_weighted(const uint32_t* d_windows, size_t nkeys, const rss_tuple4* d_tuples,
                           const uint32_t* d_weights, size_t n, uint32_t htable, uint32_t nqueues,
                           uint64_t* d_loads, hipStream_t stream) {
    int rc = launch_zero_counts(d_loads, (uint64_t)nkeys * nqueues, stream);
    if (rc || n == 0) return rc;
    DeviceInfo info;
    rc = device_info(&info);
    if (rc) return rc;
    LaunchParams p;
    memset(&p, 0, sizeof p);
    p.tuples = d_tuples;
    p.n = n;
    p.q_stride = nqueues;  // rows keep the caller's nqueues; queues >= min(H, Q) stay zero
    const uint32_t q_eff = effective_queues(htable, nqueues, nullptr);
    int qmode, hist;
    uint32_t half_bytes;  // per key of the pair kernel, as u32 bins
    const bool h_pow2 = setup_modes(&p, htable, q_eff, true, &qmode, &hist, &half_bytes,
                                    kWidePairBinBytesMax / 4, false);
    // packed tables whenever their lane-private u64 bins fit: 8 keys (H <= 256) to Q = 77,
    // 4 keys (H <= 65536) to Q = 154; else pairs of full hashes
    const bool bytes_fit = (uint64_t)q_eff * 8 * kLoadRowBytes <= kPackedBinBytesMax;
    const int lane_bits = htable <= 256u && bytes_fit ? 8 : 16;
    const uint32_t packed_keys = 64 / lane_bits;
    const uint64_t packed_bins = (uint64_t)q_eff * packed_keys * kLoadRowBytes;
    const bool packed = h_pow2 && htable <= 65536u && packed_bins <= kPackedBinBytesMax;
    const uint32_t keys_per_wg = packed ? packed_keys : 2;
    const uint32_t shmem = packed ? (uint32_t)std::max<uint64_t>(packed_bins, kPackedPrepBytes)
                                  : 4 * half_bytes;  // 2 keys x 8-byte bins
    WeightedKernelFn fn = packed   ? pick_packed(lane_bits, qmode)
                          : h_pow2 ? pick_pair<true>(qmode, hist)
                                   : pick_pair<false>(qmode, hist);
    const unsigned gx = search_grid_x(n, info.cu_count);
    const size_t max_keys = (size_t)keys_per_wg * 65535;  // grid.y limit
    for (size_t k0 = 0; k0 < nkeys; k0 += max_keys) {
        const size_t kn = nkeys - k0 < max_keys ? nkeys - k0 : max_keys;
        p.key_windows = d_windows + k0 * RSS_INPUT_BITS;
        p.counts = reinterpret_cast<unsigned long long*>(d_loads + k0 * nqueues);
        p.nkeys = (uint32_t)kn;
        hipLaunchKernelGGL(fn, dim3(gx, (unsigned)((kn + keys_per_wg - 1) / keys_per_wg)),
                           dim3(kBlock), shmem, stream, p, d_weights);
        RSS_HIP_CHECK(hipGetLastError());
    }
    return RSS_OK;
}

int launch_neighbourhood_weighted(const rss_key* key, const rss_tuple4* d_tuples,
                                  const uint32_t* d_weights, size_t n, uint32_t htable,
                                  uint32_t nqueues, uint64_t* d_loads, hipStream_t stream) {
    static_assert(RSS_KEY_NEIGHBOURS % 32 == 0, "every ng divides the rows");
    int rc = launch_zero_counts(d_loads, (uint64_t)RSS_KEY_NEIGHBOURS * nqueues, stream);
    if (rc || n == 0) return rc;
    DeviceInfo info;
    rc = device_info(&info);
    if (rc) return rc;
    LaunchParams p;
    memset(&p, 0, sizeof p);
    memcpy(p.window, key->window, sizeof p.window);
    p.tuples = d_tuples;
    p.n = n;
    p.counts = reinterpret_cast<unsigned long long*>(d_loads);
    p.q_stride = nqueues;
    const uint32_t q_eff = effective_queues(htable, nqueues, nullptr);
    int qmode, hist;
    uint32_t half_bytes;  // of one neighbour, as u32 bins
    const bool h_pow2 =
        setup_modes(&p, htable, q_eff, true, &qmode, &hist, &half_bytes, kNbrBinBytesMax / 2);
    const uint32_t ng =
        hist == HIST_GLOBAL ? 32u : neighbours_per_workgroup(2ull * half_bytes, kNbrBinBytesMax);
    p.nkeys = ng;
    const unsigned gy = RSS_KEY_NEIGHBOURS / ng;
    const unsigned gx = neighbourhood_grid_x(n, hist == HIST_PRIVATE ? q_eff : q_eff / kBinCols, gy,
                                             info.cu_count);
    hipLaunchKernelGGL(pick_nbr(hist, ng, h_pow2, qmode), dim3(gx, gy), dim3(kBlock),
                       2 * half_bytes * ng, stream, p, d_weights);
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

}  // namespace rss
