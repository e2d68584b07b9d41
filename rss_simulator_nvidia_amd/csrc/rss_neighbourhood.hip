// rss_neighbourhood.hip -- a key's single-bit-flip neighbourhood (key search's local step): the
// per-queue counts of the same device-resident tuples under each of the 128 keys that differ
// from one key in one of the bits that feed an IPv4 hash, in one launch.  No test hooks:
// compiled once for both libraries.
//
// Toeplitz is linear in the key as well as in the input: window i is key bits [i, i + 32), so
// key bit j sits at bit i + 31 - j of window i and flipping it toggles hash bit b exactly when
// input bit b + j - 31 is set.  With X the 96-bit integer whose bit i is input bit i (0 = MSB of
// the source ip; words brev(sip), brev(dip), brev(ports) from the low end) and R = X << 31,
//     hash(key ^ bit j, x) = hash(key, x) ^ ((R >> j) & 0xFFFFFFFF),   j = 0 .. 127
// for a key of >= 16 bytes (no wrap in the windows).  R has 127 bits, so j = 127 changes nothing:
// row 127 is the key itself.  A neighbour therefore costs no table of its own -- one base hash
// per tuple on the conflict-free small tables (21 ds_read_b32, 2688 B of LDS), then per
// neighbour one v_alignbit_b32, one XOR, the bucket / queue step and one LDS add.
//
// IPv6 (rss_key_neighbourhood6_device) is the same identity on nine words: X has 288 bits, R =
// X << 31 has 319 in ten words, j = 0 .. 319 and row 319 is the key itself (a 40-byte key does
// not wrap).  The base hash reads 63 small tables (8064 B), built in the kernel from the
// key's ten words -- all that a plain Toeplitz key's 288 windows hold, carried in
// LaunchParams::window[0 .. 9] -- and a group's deltas come from three of the tuple's nine
// words, picked by the uniform j0 >> 5.  One kernel template serves both (kWords = 3 / 9).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <algorithm>

#include "rss_engine.h"
#include "rss_kernel_common.h"
#include "rss_keysearch_tables.h"

namespace {

// Work split.  A workgroup (blockIdx.y) serves `ng` consecutive neighbours j0 = ng * y .. and
// histograms its grid-stride share (blockIdx.x) of the tuples for all of them; ng is a power
// of two <= 32, so the group's deltas all come from ONE pair of R's words (j0 >> 5, uniform)
// shifted by (j0 & 31) + k: the pair is picked and pre-shifted once per tuple and k is a
// constant of the unrolled loop.
// Bins.  u32, [queue][neighbour][lane column] (kBinCols = 32 columns, one per bank, as the
// packed search kernel's): a half-wave's adds never collide, the neighbour's 128-byte offset is
// the ds_add's immediate and the queue's row a multiple of a compile-time size --
// [neighbour][queue][column] would want a base register per neighbour instead.  At H = 128,
// Q = 24 a neighbour is 6 full-rate VALU instructions and one ds_add_u32.  ng is the largest
// power of two whose bins fit beside the tables:
//     ng (private bins)   32    16    8     4     2     1
//     queues up to        39    78    157   314   629   1259
// Past 1259 queues the bins lose their columns ([queue][neighbour], ng = 16 up to 2518 queues,
// 8 to 5036, 4 to 10072, 2 to 20144, 1 to 40288), and past those every (tuple, neighbour) is
// one global atomic: exact for any H, Q, only slower.  These two run one kernel body with ng
// at run time (kNG = 0).
// IPv6: 8064 B of tables leave 155776 B --
//     ng (private bins)   32    16    8     4     2     1
//     queues up to        38    76    152   304   608   1217
// then [queue][neighbour] bins with ng = 16 up to 2434 queues, 8 to 4868, 4 to 9736, 2 to 19472,
// 1 to 38944, then global atomics.
template <int kWords, int kNG, bool kHPow2, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_key_neighbourhood_kernel(const LaunchParams p) {
    __shared__ uint32_t lut[kNbrLutDwords<kWords>];
    extern __shared__ uint32_t bins[];
    const uint32_t tid = threadIdx.x;
    const uint32_t ng = kNG ? (uint32_t)kNG : p.nkeys;
    const uint32_t j0 = ng * blockIdx.y;
    const uint32_t word = j0 >> 5, s0 = j0 & 31u;
    if constexpr (kWords == 3) build_small_lut(lut, p.window, tid);
    else build_small_lut6(lut, p.window, tid);
    const uint32_t nbins =
        kHist == HIST_PRIVATE ? p.Q * ng * kBinCols : (kHist == HIST_SHARED ? p.Q * ng : 0u);
    for (uint32_t e = tid; e < nbins; e += kBlock) bins[e] = 0;
    __syncthreads();

    char* bins_colb = reinterpret_cast<char*>(bins + (tid & (kBinCols - 1)));
    constexpr uint32_t kRowBytes = kNG * kBinCols * 4;  // private bins: one queue's row
    // QM_FAST8 (H <= 256) folded into the row's byte offset as in the packed search kernel:
    // q * row = b * row - d * (Q * row), d = floor(b / Q) -- two full-rate 24-bit multiplies,
    // the second a v_mad_i32_i24, where queue_of's b - d * Q compiles to a quarter-rate
    // v_mul_lo_u32 (Q * row <= 161152 and b * row < 2^20 fit 24 bits)
    const int neg_q_row = -(int)(p.Q * kRowBytes);
    unsigned long long* rows = p.counts + (size_t)j0 * p.q_stride;  // row k at k * q_stride
    auto count = [&](const uint32_t* w) {  // one tuple's kWords words
        uint32_t h;
        uint2 span;
        if constexpr (kWords == 3) {
            h = toeplitz_hash_small(lut, w[0], w[1], w[2]);
            span = flip_span(w[0], w[1], w[2], word, s0);
        } else {
            h = toeplitz_hash_small6(lut, w);
            span = flip_span6(w, word, s0);
        }
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
                __hip_atomic_fetch_add(reinterpret_cast<uint32_t*>(bins_colb + row) + k * kBinCols,
                                       1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else if constexpr (kHist == HIST_SHARED) {
                __hip_atomic_fetch_add(&bins[queue_of<kQMode>(b, p) * ng + k], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                atomicAdd(&rows[(size_t)k * p.q_stride + queue_of<kQMode>(b, p)], 1ull);
            }
        };
        if constexpr (kNG != 0) {
#pragma unroll
            for (uint32_t k = 0; k < (uint32_t)kNG; ++k) neighbour(k);
        } else {
            for (uint32_t k = 0; k < ng; ++k) neighbour(k);
        }
    };
    const uint64_t gtid = (uint64_t)blockIdx.x * kBlock + tid;
    const uint64_t gstride = (uint64_t)gridDim.x * kBlock;
    uint64_t tail_begin = 0;
    if (((uintptr_t)p.tuples & 15u) == 0) {  // 16-byte aligned: four tuples per lane
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.tuples);
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
#pragma unroll
            for (int u = 0; u < 4; ++u) count(w + kWords * u);
        }
        tail_begin = ngroups << 2;
    }
    for (uint64_t i = tail_begin + gtid; i < p.n; i += gstride) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(p.tuples) + kWords * i;
        uint32_t w[kWords];
#pragma unroll
        for (int k = 0; k < kWords; ++k) w[k] = t[k];
        count(w);
    }
    if constexpr (kHist != HIST_GLOBAL) {
        __syncthreads();
        const uint32_t ng_shift = 31 - __clz(ng);
        for (uint32_t e = tid; e < p.Q * ng; e += kBlock) {  // e = q * ng + k
            uint32_t s;
            if constexpr (kHist == HIST_PRIVATE) {
                s = 0;
                for (uint32_t c = 0; c < kBinCols; ++c)
                    s += bins[e * kBinCols + ((c + e) & (kBinCols - 1))];
            } else {
                s = bins[e];
            }
            if (s)
                atomicAdd(&rows[(size_t)(e & (ng - 1)) * p.q_stride + (e >> ng_shift)],
                          (unsigned long long)s);
        }
    }
}

// the counts are overwritten: cleared by a kernel, so that the entry point can be captured
// into a graph like any other launch
__global__ __launch_bounds__(kBlock) void rss_zero_counts_kernel(unsigned long long* counts,
                                                                 uint64_t n) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) counts[i] = 0;
}

template <int kWords, int kNG, bool kHPow2, int kHist>
KernelFn pick_nbr_qmode(int qmode) {
    switch (qmode) {
        case QM_MASK: return rss_key_neighbourhood_kernel<kWords, kNG, kHPow2, QM_MASK, kHist>;
        case QM_FAST8: return rss_key_neighbourhood_kernel<kWords, kNG, kHPow2, QM_FAST8, kHist>;
        case QM_FAST16: return rss_key_neighbourhood_kernel<kWords, kNG, kHPow2, QM_FAST16, kHist>;
        default: return rss_key_neighbourhood_kernel<kWords, kNG, kHPow2, QM_FAST32, kHist>;
    }
}

template <int kWords, int kNG, int kHist>
KernelFn pick_nbr_modes(bool h_pow2, int qmode) {
    return h_pow2 ? pick_nbr_qmode<kWords, kNG, true, kHist>(qmode)
                  : pick_nbr_qmode<kWords, kNG, false, kHist>(qmode);
}

template <int kWords>
KernelFn pick_nbr(int hist, uint32_t ng, bool h_pow2, int qmode) {
    if (hist == HIST_SHARED) return pick_nbr_modes<kWords, 0, HIST_SHARED>(h_pow2, qmode);
    if (hist != HIST_PRIVATE) return pick_nbr_modes<kWords, 0, HIST_GLOBAL>(h_pow2, qmode);
    switch (ng) {
        case 32: return pick_nbr_modes<kWords, 32, HIST_PRIVATE>(h_pow2, qmode);
        case 16: return pick_nbr_modes<kWords, 16, HIST_PRIVATE>(h_pow2, qmode);
        case 8: return pick_nbr_modes<kWords, 8, HIST_PRIVATE>(h_pow2, qmode);
        case 4: return pick_nbr_modes<kWords, 4, HIST_PRIVATE>(h_pow2, qmode);
        case 2: return pick_nbr_modes<kWords, 2, HIST_PRIVATE>(h_pow2, qmode);
        default: return pick_nbr_modes<kWords, 1, HIST_PRIVATE>(h_pow2, qmode);
    }
}

}  // namespace

// ------------------------------------------------------ launcher (rss_engine.h) --
namespace rss {

int launch_zero_counts(uint64_t* d_counts, uint64_t cells, hipStream_t stream) {
    DeviceInfo info;
    int rc = device_info(&info);
    if (rc) return rc;
    const unsigned zero_grid = (unsigned)std::max<uint64_t>(
        1, std::min<uint64_t>((cells + kBlock - 1) / kBlock, 4u * (unsigned)info.cu_count));
    hipLaunchKernelGGL(rss_zero_counts_kernel, dim3(zero_grid), dim3(kBlock), 0, stream,
                       reinterpret_cast<unsigned long long*>(d_counts), cells);
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

// both entries: clear, then one launch of the kWords kernel over `neighbours` rows; p holds
// the key (window) and the tuples
template <int kWords>
static int launch_neighbourhood_rows(LaunchParams& p, uint32_t neighbours, uint32_t budget,
                                     uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                                     hipStream_t stream) {
    int rc = launch_zero_counts(d_counts, (uint64_t)neighbours * nqueues, stream);
    if (rc || p.n == 0) return rc;
    DeviceInfo info;
    rc = device_info(&info);
    if (rc) return rc;
    p.counts = reinterpret_cast<unsigned long long*>(d_counts);
    p.q_stride = nqueues;  // rows keep the caller's nqueues; queues >= min(H, Q) stay zero
    const uint32_t q_eff = effective_queues(htable, nqueues, nullptr);
    int qmode, hist;
    uint32_t bin_bytes;  // of one neighbour
    const bool h_pow2 = setup_modes(&p, htable, q_eff, true, &qmode, &hist, &bin_bytes, budget);
    const uint32_t ng = hist == HIST_GLOBAL ? 32u : neighbours_per_workgroup(bin_bytes, budget);
    p.nkeys = ng;
    const unsigned gy = neighbours / ng;
    const unsigned gx = neighbourhood_grid_x(p.n, hist == HIST_PRIVATE ? q_eff : q_eff / kBinCols, gy,
                                             info.cu_count);
    hipLaunchKernelGGL(pick_nbr<kWords>(hist, ng, h_pow2, qmode), dim3(gx, gy), dim3(kBlock),
                       bin_bytes * ng, stream, p);
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

int launch_neighbourhood(const rss_key* key, const rss_tuple4* d_tuples, size_t n, uint32_t htable,
                         uint32_t nqueues, uint64_t* d_counts, hipStream_t stream) {
    LaunchParams p;
    memset(&p, 0, sizeof p);
    memcpy(p.window, key->window, sizeof p.window);
    p.tuples = d_tuples;
    p.n = n;
    return launch_neighbourhood_rows<3>(p, RSS_KEY_NEIGHBOURS, kNbrBinBytesMax, htable, nqueues,
                                        d_counts, stream);
}

int launch_neighbourhood6(const rss_key6* key, const rss_tuple6* d_tuples, size_t n,
                          uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                          hipStream_t stream) {
    static_assert(RSS_KEY6_NEIGHBOURS % 32 == 0, "every ng divides the rows");
    LaunchParams p;
    memset(&p, 0, sizeof p);
    // a plain Toeplitz key (checked by the caller): window 32 k is key word k; word 9 = key
    // bits [288, 319) from the last window (bit 319 feeds no hash)
    for (int k = 0; k < kWords6; ++k) p.window[k] = key->window[32 * k];
    p.window[kWords6] = key->window[RSS_INPUT6_BITS - 1] << 1;
    p.tuples = reinterpret_cast<const rss_tuple4*>(d_tuples);  // read as dwords / uint4 only
    p.n = n;
    return launch_neighbourhood_rows<kWords6>(p, RSS_KEY6_NEIGHBOURS, kNbr6BinBytesMax, htable,
                                              nqueues, d_counts, stream);
}

}  // namespace rss
