// rss_keysearch6.hip -- key search over IPv6 tuples: the per-queue counts of the same
// device-resident 36-byte tuples under many 40-byte keys in one launch (rss_key_search6_device),
// the packed search kernel's idea (rss_keysearch.hip) carried from three input words to nine.
// No test hooks: compiled once for both libraries.
//
// Tables.  A table index depends only on the tuple, so one table serves several keys.  Word k
// of the tuple (w[0] .. w[8]) is cut LSB first into fields of 5, 5, 5, 5, 5, 5 and 2 bits
// (the small tables of rss_kernel_common.h) and table 7k + j is indexed by field j: 63 tables
// of at most 32 entries.  An entry is 8 bytes, so a table is 256 B and covers the 64 banks of
// a ds_read_b64 exactly once -- every entry sits on its own bank pair and a random index never
// conflicts.  63 x 256 B = 16128 B leave 147712 B of the 160 KiB LDS to the bins.  An entry
// holds, for the input bits set in its index, the XOR of the windows of
//   * 8 keys, low byte each       (kLaneBits = 8:  power-of-two H <= 256),
//   * 4 keys, low half-word each  (kLaneBits = 16: power-of-two H <= 65536) or
//   * 2 keys, all 32 bits         (kLaneBits = 32: any H)
// -- for a power-of-two H the bucket is the low log2(H) bits of the hash and the low bits of a
// XOR are the XOR of the low bits, so a lane needs no more of a key than that.
// Per tuple: 63 ds_read_b64 and 62 three-input XORs per half whatever the lane width; then per
// key a bit-field extract (32-bit lanes: the mask or the Lemire remainder), the queue step and
// one LDS add.
// Bins.  u32, [queue][key][lane column] with kBinCols = 32 columns: a half-wave's adds never
// collide, the key's 128-byte offset is the ds_add's immediate and the queue's row a shift.
//     keys per workgroup     8      4      2
//     private bins up to Q   144    288    577
// Past 577 queues the pair kernel's bins lose their columns ([queue][key], up to 18464 queues)
// and past those every (tuple, key) is one global atomic: exact for any H, Q, only slower.
// Work split.  blockIdx.y selects the key group, blockIdx.x the grid-stride share of the
// tuples; the flows are re-read from the on-die cache by every key group.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <algorithm>

#include "rss_engine.h"
#include "rss_kernel_common.h"

namespace {

constexpr int kWords6 = RSS_INPUT6_BITS / 32;                      // 9
constexpr int kTables6 = kWords6 * kSmallFields;                   // 63
constexpr uint32_t kLut6Entries = kTables6 * 32;                   // 2016
constexpr uint32_t kLut6Bytes = kLut6Entries * 8;                  // 16128
constexpr uint32_t kBins6BytesMax = kLdsBytes - kLut6Bytes;        // 147712
constexpr uint32_t kPrep6Bytes = RSS_INPUT6_BITS * 8;              // packed windows, before the bins
static_assert(kLut6Bytes == 16128 && kBins6BytesMax == 147712, "IPv6 key-search LDS split");
static_assert((kTables6 - 1) * 256 + 31 * 8 < 65536, "every table within the ds_read immediate");

// table 7k + j's 8-byte term for word w (= word k): the field moved to byte offset 8 * field
template <int kT>
__device__ __forceinline__ uint2 term6(const char* lut, uint32_t w) {
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
__device__ __forceinline__ uint2 word6(const char* lut, uint32_t w) {  // 7 terms
    const uint2 t0 = term6<kBase + 0>(lut, w), t1 = term6<kBase + 1>(lut, w);
    const uint2 t2 = term6<kBase + 2>(lut, w), t3 = term6<kBase + 3>(lut, w);
    const uint2 t4 = term6<kBase + 4>(lut, w), t5 = term6<kBase + 5>(lut, w);
    const uint2 t6 = term6<kBase + 6>(lut, w);
    return make_uint2(xor3(xor3(t0.x, t1.x, t2.x), xor3(t3.x, t4.x, t5.x), t6.x),
                      xor3(xor3(t0.y, t1.y, t2.y), xor3(t3.y, t4.y, t5.y), t6.y));
}

// the packed hashes of one tuple: every lane holds its key's hash (its low kLaneBits)
__device__ __forceinline__ uint2 toeplitz_hash6_packed(const uint2* __restrict__ lut,
                                                       const uint32_t* w) {
    const char* b = reinterpret_cast<const char*>(lut);
    const uint2 a0 = word6<0>(b, w[0]), a1 = word6<7>(b, w[1]), a2 = word6<14>(b, w[2]);
    const uint2 a3 = word6<21>(b, w[3]), a4 = word6<28>(b, w[4]), a5 = word6<35>(b, w[5]);
    const uint2 a6 = word6<42>(b, w[6]), a7 = word6<49>(b, w[7]), a8 = word6<56>(b, w[8]);
    return make_uint2(xor3(xor3(a0.x, a1.x, a2.x), xor3(a3.x, a4.x, a5.x), xor3(a6.x, a7.x, a8.x)),
                      xor3(xor3(a0.y, a1.y, a2.y), xor3(a3.y, a4.y, a5.y), xor3(a6.y, a7.y, a8.y)));
}

// kLaneBits 8 / 16 run with private bins only (kHPow2, HIST_PRIVATE); 32 takes every mode.
template <int kLaneBits, bool kHPow2, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_key_search6_kernel(const LaunchParams p) {
    constexpr uint32_t kKeys = 64 / kLaneBits;
    static_assert(kLaneBits == 32 || (kHPow2 && kHist == HIST_PRIVATE), "packed lanes: pow2 H, private bins");
    __shared__ uint2 lut[kLut6Entries];
    extern __shared__ __attribute__((aligned(16))) uint32_t bins[];
    const uint32_t tid = threadIdx.x;
    const uint32_t key0 = kKeys * blockIdx.y;

    // 1. pack: lane k of packed[i] = low kLaneBits of key (key0 + k)'s window i (a key past
    //    the end repeats the last key; its counts are discarded)
    uint2* packed = reinterpret_cast<uint2*>(bins);
    if (tid < RSS_INPUT6_BITS) {
        uint32_t lane[2] = {0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < kKeys; ++k) {
            const uint32_t key = min(key0 + k, p.nkeys - 1);
            const uint32_t w = p.key_windows[(size_t)RSS_INPUT6_BITS * key + tid] &
                               (uint32_t)((1ull << kLaneBits) - 1);
            lane[(k * kLaneBits) >> 5] |= w << ((k * kLaneBits) & 31u);
        }
        packed[tid] = make_uint2(lane[0], lane[1]);
    }
    __syncthreads();
    // 2. tables: entry e = 32 t + v = the XOR of the packed windows of the input bits set in v
    for (uint32_t e = tid; e < kLut6Entries; e += kBlock) {
        const int t = (int)(e >> 5);
        const uint32_t v = e & 31u;
        const int width = small_width(t % kSmallFields);
        uint32_t a = 0, b = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            if (j < width && ((v >> j) & 1u)) {
                const uint2 w = packed[small_slice_bit(t, j)];
                a ^= w.x;
                b ^= w.y;
            }
        }
        lut[e] = (v >> width) ? make_uint2(0u, 0u) : make_uint2(a, b);
    }
    __syncthreads();  // packed windows are dead: the region becomes bins
    const uint32_t nbins = kHist == HIST_PRIVATE ? p.Q * kKeys * kBinCols
                                                 : (kHist == HIST_SHARED ? p.Q * kKeys : 0u);
    for (uint32_t e = tid; e < nbins; e += kBlock) bins[e] = 0;
    __syncthreads();

    char* bins_colb = reinterpret_cast<char*>(bins + (tid & (kBinCols - 1)));
    const uint32_t hbits = 31 - __clz(p.H);  // log2(H) (packed lanes)
    constexpr uint32_t kRowShift = kLaneBits == 8 ? 10 : (kLaneBits == 16 ? 9 : 8);  // log2(kKeys * kBinCols * 4)
    // byte-lane queue step folded into the bin address as in the IPv4 packed kernel:
    // q * 2^kRowShift = (b << kRowShift) - d * (Q << kRowShift), d = floor(b / Q)
    const int neg_q_row = -(int)(p.Q << kRowShift);
    const uint32_t lane_mask4 = (p.H - 1) * 0x01010101u;
    const bool has_b = key0 + 1 < p.nkeys;  // pair kernel: the second key is real
    unsigned long long* rows = p.counts + (size_t)key0 * p.q_stride;
    auto count = [&](uint2 x) {
        if constexpr (kLaneBits == 8) {
            x.x &= lane_mask4;
            x.y &= lane_mask4;
        }
#pragma unroll
        for (uint32_t k = 0; k < kKeys; ++k) {
            const uint32_t word = (k * kLaneBits) < 32 ? x.x : x.y;
            uint32_t b;
            if constexpr (kLaneBits == 8)
                b = (word >> ((k * 8) & 31)) & 0xFFu;
            else if constexpr (kLaneBits == 16)
                b = __builtin_amdgcn_ubfe(word, (k * 16) & 31, hbits);
            else
                b = bucket_of<kHPow2>(word, p);
            if constexpr (kHist == HIST_PRIVATE) {
                uint32_t row;
                if constexpr (kLaneBits == 8 && kQMode == QM_FAST16) {
                    const uint32_t d = __umul24(b, p.q_m16) >> 16;
                    row = (uint32_t)__mul24((int)d, neg_q_row) + (b << kRowShift);
                } else {
                    row = queue_of<kQMode>(b, p) << kRowShift;
                }
                __hip_atomic_fetch_add(reinterpret_cast<uint32_t*>(bins_colb + row) + k * kBinCols, 1u,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else if constexpr (kHist == HIST_SHARED) {
                __hip_atomic_fetch_add(&bins[queue_of<kQMode>(b, p) * kKeys + k], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                if (k == 0 || has_b)
                    atomicAdd(&rows[(size_t)k * p.q_stride + queue_of<kQMode>(b, p)], 1ull);
            }
        }
    };
    const uint64_t gtid = (uint64_t)blockIdx.x * kBlock + tid;
    const uint64_t gstride = (uint64_t)gridDim.x * kBlock;
    uint64_t tail_begin = 0;
    if (((uintptr_t)p.tuples & 15u) == 0) {  // 16-byte aligned: four tuples (144 B) per lane
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.tuples);
        const uint64_t ngroups = p.n >> 2;
        for (uint64_t g = gtid; g < ngroups; g += gstride) {
            uint32_t w[4 * kWords6];
#pragma unroll
            for (int i = 0; i < kWords6; ++i) {
                const uint4 x = src[kWords6 * g + i];
                w[4 * i + 0] = x.x;
                w[4 * i + 1] = x.y;
                w[4 * i + 2] = x.z;
                w[4 * i + 3] = x.w;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) count(toeplitz_hash6_packed(lut, w + kWords6 * u));
        }
        tail_begin = ngroups << 2;
    }
    for (uint64_t i = tail_begin + gtid; i < p.n; i += gstride) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(p.tuples) + kWords6 * i;
        uint32_t w[kWords6];
#pragma unroll
        for (int k = 0; k < kWords6; ++k) w[k] = t[k];
        count(toeplitz_hash6_packed(lut, w));
    }
    if constexpr (kHist != HIST_GLOBAL) {
        __syncthreads();
        for (uint32_t e = tid; e < p.Q * kKeys; e += kBlock) {  // e = q * kKeys + k
            const uint32_t q = e / kKeys, k = e % kKeys;
            if (key0 + k >= p.nkeys) continue;
            uint32_t s;
            if constexpr (kHist == HIST_PRIVATE) {
                s = 0;
                for (uint32_t c = 0; c < kBinCols; ++c)
                    s += bins[e * kBinCols + ((c + e) & (kBinCols - 1))];
            } else {
                s = bins[e];
            }
            if (s) atomicAdd(&rows[(size_t)k * p.q_stride + q], (unsigned long long)s);
        }
    }
}

template <bool kHPow2, int kQMode>
KernelFn pick_pair6_hist(int hist) {
    switch (hist) {
        case HIST_PRIVATE: return rss_key_search6_kernel<32, kHPow2, kQMode, HIST_PRIVATE>;
        case HIST_SHARED: return rss_key_search6_kernel<32, kHPow2, kQMode, HIST_SHARED>;
        default: return rss_key_search6_kernel<32, kHPow2, kQMode, HIST_GLOBAL>;
    }
}

template <bool kHPow2>
KernelFn pick_pair6(int qmode, int hist) {
    switch (qmode) {
        case QM_MASK: return pick_pair6_hist<kHPow2, QM_MASK>(hist);
        case QM_FAST16: return pick_pair6_hist<kHPow2, QM_FAST16>(hist);
        default: return pick_pair6_hist<kHPow2, QM_FAST32>(hist);
    }
}

KernelFn pick_packed6(int lane_bits, int qmode) {
    if (lane_bits == 8)
        return qmode == QM_MASK ? rss_key_search6_kernel<8, true, QM_MASK, HIST_PRIVATE>
                                : rss_key_search6_kernel<8, true, QM_FAST16, HIST_PRIVATE>;
    return qmode == QM_MASK ? rss_key_search6_kernel<16, true, QM_MASK, HIST_PRIVATE>
                            : rss_key_search6_kernel<16, true, QM_FAST16, HIST_PRIVATE>;
}

// Workgroups along x.  A workgroup's fixed cost is its 16 KiB of tables (two entries per lane)
// and its bins, cleared and summed again: at most 147712 B / 1024 lanes = 36 dwords per lane
// each way -- so 64 tuples per lane keep it near a tenth of the 63 reads and 2 .. 8 adds per
// tuple.  No more than one workgroup per CU along x: the key groups along y fill the device.
inline unsigned search6_grid_x(size_t n, int cu_count) {
    const uint64_t slices = (n + (1u << 16) - 1) >> 16;
    return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(slices, (uint64_t)cu_count));
}

}  // namespace

// ------------------------------------------------------ launcher (rss_engine.h) --
namespace rss {

int launch_search6(const uint32_t* d_windows, size_t nkeys, const rss_tuple6* d_tuples, size_t n,
                   uint32_t htable, uint32_t nqueues, uint64_t* d_counts, hipStream_t stream) {
    int rc = launch_zero_counts(d_counts, (uint64_t)nkeys * nqueues, stream);
    if (rc || n == 0) return rc;
    LaunchParams p;
    memset(&p, 0, sizeof p);
    p.tuples = reinterpret_cast<const rss_tuple4*>(d_tuples);  // read as dwords / uint4 only
    p.n = n;
    p.q_stride = nqueues;  // rows keep the caller's nqueues; queues >= min(H, Q) stay zero
    const uint32_t q_eff = effective_queues(htable, nqueues, nullptr);
    int qmode, hist;
    uint32_t bin_bytes;  // per key of a pair
    const bool h_pow2 = setup_modes(&p, htable, q_eff, true, &qmode, &hist, &bin_bytes,
                                    kBins6BytesMax / 2, false);
    DeviceInfo info;
    rc = device_info(&info);
    if (rc) return rc;
    // 8 keys per table entry for a power-of-two H <= 256 while their private bins fit
    // (Q <= 144), 4 for H <= 65536 (Q <= 288); else pairs of full hashes
    const uint64_t row_bytes = (uint64_t)q_eff * kBinCols * 4;  // one key's private bins
    int lane_bits = 32;
    if (h_pow2 && htable <= 256u && row_bytes * 8 <= kBins6BytesMax) lane_bits = 8;
    else if (h_pow2 && htable <= 65536u && row_bytes * 4 <= kBins6BytesMax) lane_bits = 16;
    const uint32_t keys_per_wg = 64 / lane_bits;
    const uint64_t bins = lane_bits == 32 ? 2ull * bin_bytes : row_bytes * keys_per_wg;
    KernelFn fn = lane_bits != 32 ? pick_packed6(lane_bits, qmode)
                : h_pow2          ? pick_pair6<true>(qmode, hist)
                                  : pick_pair6<false>(qmode, hist);
    const uint32_t shmem = (uint32_t)std::max<uint64_t>(bins, kPrep6Bytes);
    const unsigned gx = search6_grid_x(n, info.cu_count);
    const size_t max_keys = (size_t)keys_per_wg * 65535;  // grid.y limit
    for (size_t k0 = 0; k0 < nkeys; k0 += max_keys) {
        const size_t kn = nkeys - k0 < max_keys ? nkeys - k0 : max_keys;
        p.key_windows = d_windows + k0 * RSS_INPUT6_BITS;
        p.counts = reinterpret_cast<unsigned long long*>(d_counts + k0 * nqueues);
        p.nkeys = (uint32_t)kn;
        hipLaunchKernelGGL(fn, dim3(gx, (unsigned)((kn + keys_per_wg - 1) / keys_per_wg)),
                           dim3(kBlock), shmem, stream, p);
        RSS_HIP_CHECK(hipGetLastError());
    }
    return RSS_OK;
}

}  // namespace rss
