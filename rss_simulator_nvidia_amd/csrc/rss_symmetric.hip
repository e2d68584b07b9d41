// rss_symmetric.hip -- symmetric RSS: the per-queue loads of a flow set under every key with a
// 16-bit period (rss_symmetric_fold_device, rss_symmetric_search_device).  Such a key hashes
// both directions of a connection to one queue; DPDK's 6d:5a:6d:5a:... is one of the 65536.
// No test hooks: compiled once for both libraries.
//
// The identity.  Key bit i of a periodic key is bit 15 - i % 16 of its pattern p, so the
// window of input bit i is rotl16(p, i % 16) twice over, and a word's bit at position r from
// its half-word's MSB always meets rotation r, whichever word or half it sits in.  With f the
// XOR of the tuple's 16-bit half-words and f_r = bit 15 - r of f,
//     g(f, p) = XOR over r with f_r set of rotl16(p, r),     hash = (g << 16) | g.
// Every field is a multiple of 16 bits, so a field selection only masks half-words out of f.
// A flow set -- IPv4 or IPv6, weighted or not, of any size -- is therefore a 65536-bin
// histogram of fold values, and ranking every pattern is 2^32 (fold, pattern) evaluations.
//
// rss_symmetric_fold_kernel.  65536 u64 bins are 512 KiB, so blockIdx.y = 0..3 owns the fold
// values whose top two bits are y in 16384 u64 LDS bins (128 KiB); blockIdx.x takes a
// grid-stride share of the tuples and a lane whose f is another quarter's skips the add.  Every
// add is one ds_add_u64 of the weight (1 without weights): exact for any u32 weights and any
// n.  The flush is one global 64-bit atomic per non-zero bin.  Input as the weighted kernels':
// four tuples per lane through dwordx4 loads (3 or 9, plus one of weights) when tuples and
// weights are 16-byte aligned, else -- and for the n % 4 tail -- one tuple per lane through
// dword loads; a uniform branch on the pointers.
//
// rss_symmetric_search_kernel.  blockIdx.y serves a group of 8 (byte lanes: power-of-two
// H <= 256, where the bucket is g's low bits) or 4 (half-word lanes: any H) consecutive
// patterns, blockIdx.x a 1024-aligned share of the fold values.  f is cut 5 + 5 + 5 + 1:
// three 32-entry tables of 8-byte entries (256 B each: the 64 banks once, so no read can
// conflict), lane k of entry v of table t the XOR of pattern k's rotations 15 - (5 t + b)
// over the bits b set in v, and the top bit selects the packed patterns themselves (rotation
// 0).  A lane's fold values are f0 + tid + 1024 i, so its first two table reads do not depend
// on i and leave the loop: one ds_read_b64, one select and two v_bitop3 per fold value hash it
// under the whole group.  The rotation identity g(f, rotl16(p, s)) = rotl16(g(f, p), s) is not
// used: it would trade that one read for scattered pattern rows (p's rotations are not
// consecutive patterns), and the read is one LDS access against the group's 8 (4) adds.
// Bins are u64, one ds_add_u64 of folds[f] each (a lane skips f with folds[f] == 0), in the
// weighted kernels' layout [queue][pattern][32 lane columns], 256 B a row, the queue step
// folded into the row address; tiers by the LDS beside the 1 KiB of tables (162816 B):
//   byte lanes, 8 patterns, lane-private        Q <= 79    (power-of-two H <= 256)
//   half-word lanes, 4 patterns, lane-private   Q <= 159
//   half-word lanes, shared [pattern][queue]    Q <= 5088
//   half-word lanes, one global 64-bit atomic per (fold, pattern) past that
// (Q = min(H, nqueues)).  A last partial group neither adds nor flushes its padding patterns.
// The loads are cleared by rss_zero_counts_kernel in the same call: graph-capturable.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <algorithm>

#include "rss_engine.h"
#include "rss_kernel_common.h"
#include "rss_keysearch_tables.h"

namespace {

constexpr uint32_t kFoldQuarter = RSS_SYMMETRIC_PATTERNS / 4;       // fold values per blockIdx.y
constexpr uint32_t kFoldBinBytes = kFoldQuarter * 8;                // 128 KiB of u64 bins
constexpr uint32_t kSymLutBytes = 1024;                             // 3 x 256 B + the select entry
constexpr uint32_t kSymBinBytesMax = kLdsBytes - kSymLutBytes;      // 162816
constexpr uint32_t kSymSelect = 96;                                 // lut entry of rotation 0
static_assert(kFoldBinBytes <= kLdsBytes, "a quarter of the fold bins fits the LDS");
static_assert(RSS_SYMMETRIC_PATTERNS % (64 * kBlock) == 0, "x shares are multiples of kBlock");

struct FoldMasks {
    uint32_t w[9];  // the selected fields' bits of each tuple word
};

__device__ __forceinline__ void lds_add_u64(u64* bin, u64 v) {  // ds_add_u64
    __hip_atomic_fetch_add(bin, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// ----------------------------------------------------------------- fold histogram --
template <int kWords>
__global__ __launch_bounds__(kBlock) void rss_symmetric_fold_kernel(
    const uint32_t* __restrict__ tuples, const uint32_t* __restrict__ weights, const uint64_t n,
    u64* __restrict__ folds, const FoldMasks m) {
    extern __shared__ u64 bins[];
    const uint32_t tid = threadIdx.x;
    const uint32_t quarter = blockIdx.y;
    for (uint32_t e = tid; e < kFoldQuarter; e += kBlock) bins[e] = 0;
    __syncthreads();

    auto add = [&](uint32_t x, uint32_t weight) {  // x: XOR of the tuple's masked words
        const uint32_t f = (x >> 16) ^ (x & 0xFFFFu);
        if ((f >> 14) == quarter) lds_add_u64(&bins[f & (kFoldQuarter - 1)], weight);
    };
    const uint64_t gtid = (uint64_t)blockIdx.x * kBlock + tid;
    const uint64_t gstride = (uint64_t)gridDim.x * kBlock;
    uint64_t tail_begin = 0;
    if ((((uintptr_t)tuples | (uintptr_t)weights) & 15u) == 0) {  // uniform (NULL weights: aligned)
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(tuples);
        const uint4* __restrict__ wsrc = reinterpret_cast<const uint4*>(weights);
        const uint64_t ngroups = n >> 2;
        for (uint64_t g = gtid; g < ngroups; g += gstride) {
            uint32_t v[4 * kWords];  // four tuples = kWords dwordx4
#pragma unroll
            for (int j = 0; j < kWords; ++j) {
                const uint4 a = src[kWords * g + j];
                v[4 * j + 0] = a.x;
                v[4 * j + 1] = a.y;
                v[4 * j + 2] = a.z;
                v[4 * j + 3] = a.w;
            }
            const uint4 w = wsrc ? wsrc[g] : make_uint4(1u, 1u, 1u, 1u);
            const uint32_t wt[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                uint32_t x = 0;
#pragma unroll
                for (int k = 0; k < kWords; ++k) x ^= v[t * kWords + k] & m.w[k];
                add(x, wt[t]);
            }
        }
        tail_begin = ngroups << 2;
    }
    for (uint64_t i = tail_begin + gtid; i < n; i += gstride) {
        const uint32_t* t = tuples + kWords * i;
        uint32_t x = 0;
#pragma unroll
        for (int k = 0; k < kWords; ++k) x ^= t[k] & m.w[k];
        add(x, weights ? weights[i] : 1u);
    }
    __syncthreads();
    u64* out = folds + (size_t)quarter * kFoldQuarter;
    for (uint32_t e = tid; e < kFoldQuarter; e += kBlock) {
        const u64 s = bins[e];
        if (s) atomicAdd(&out[e], s);
    }
}

// ------------------------------------------------------------------- pattern scan --
__device__ __forceinline__ uint32_t rotl16(uint32_t p, uint32_t r) {  // p < 2^16, r < 16
    return ((p << r) | (p >> (16u - r))) & 0xFFFFu;
}

template <int kLaneBits, bool kHPow2, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_symmetric_search_kernel(
    const LaunchParams p, const u64* __restrict__ folds, const uint32_t first) {
    constexpr uint32_t kPat = 64 / kLaneBits;
    static_assert(kLaneBits == 16 || (kHPow2 && kHist == HIST_PRIVATE), "byte lanes: H <= 256");
    __shared__ uint2 lut[kSymLutBytes / 8];
    extern __shared__ u64 loads[];
    const uint32_t tid = threadIdx.x;
    const uint32_t k0 = kPat * blockIdx.y;
    const uint32_t nk = min(kPat, p.nkeys - k0);  // a last group's padding is never counted

    if (tid <= kSymSelect) {  // entry v of table t, or the select entry (rotation 0)
        const uint32_t t = tid >> 5, v = tid & 31u;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (uint32_t k = 0; k < kPat; ++k) {
            const uint32_t pat = (first + k0 + k) & 0xFFFFu;
            uint32_t g = tid == kSymSelect ? pat : 0u;
#pragma unroll
            for (uint32_t b = 0; b < 5; ++b)  // fold bit 5 t + b is f_r with r = 15 - (5 t + b)
                if (tid < kSymSelect && ((v >> b) & 1u)) g ^= rotl16(pat, 15u - (5u * t + b));
            g &= (1u << kLaneBits) - 1u;
            const uint32_t shift = k * kLaneBits;
            if (shift < 32) lo |= g << shift;
            else hi |= g << (shift - 32);
        }
        lut[tid] = make_uint2(lo, hi);
    }
    const uint32_t nrows = p.Q * kPat;
    const uint32_t nbins =
        kHist == HIST_PRIVATE ? nrows * kBinCols : (kHist == HIST_SHARED ? nrows : 0u);
    for (uint32_t e = tid; e < nbins; e += kBlock) loads[e] = 0;
    __syncthreads();

    char* col = reinterpret_cast<char*>(loads + (tid & (kBinCols - 1)));
    constexpr uint32_t kRowShift = kLaneBits == 8 ? 11 : 10;  // log2(kPat * kLoadRowBytes)
    // byte lanes: q * 2^kRowShift = (b << kRowShift) - d * (Q << kRowShift), d = floor(b / Q):
    // two full-rate 24-bit multiplies (Q <= 79 rows of 2 KiB and b < 256 fit 24 bits)
    const int neg_q_row = -(int)(p.Q << kRowShift);
    const uint32_t lane_mask4 = (p.H - 1) * 0x01010101u;
    u64* rows = p.counts + (size_t)k0 * p.q_stride;  // row k at k * q_stride

    const uint32_t per_x = RSS_SYMMETRIC_PATTERNS / gridDim.x;  // a multiple of kBlock
    const uint32_t f0 = blockIdx.x * per_x;
    // f = f0 + tid + 1024 i: fold bits 0..9 are the lane's own, so two of the three reads hoist
    const uint2 ta = lut[tid & 31u], tb = lut[32u + (tid >> 5)];
    const uint2 base = make_uint2(ta.x ^ tb.x, ta.y ^ tb.y);
    const uint2 sel = lut[kSymSelect];
    for (uint32_t f = f0 + tid; f < f0 + per_x; f += kBlock) {
        const u64 weight = folds[f];
        if (!weight) continue;
        const uint2 tc = lut[64u + ((f >> 10) & 31u)];
        const bool top = (f >> 15) != 0;
        uint2 x = make_uint2(xor3(base.x, tc.x, top ? sel.x : 0u), xor3(base.y, tc.y, top ? sel.y : 0u));
        if constexpr (kLaneBits == 8) {
            x.x &= lane_mask4;
            x.y &= lane_mask4;
        }
#pragma unroll
        for (uint32_t k = 0; k < kPat; ++k) {
            if (k >= nk) break;  // uniform
            const uint32_t word = (k * kLaneBits) < 32 ? x.x : x.y;
            uint32_t b;
            if constexpr (kLaneBits == 8) {
                b = (word >> ((k * 8) & 31)) & 0xFFu;
            } else {
                const uint32_t g = (word >> ((k * 16) & 31)) & 0xFFFFu;
                b = bucket_of<kHPow2>(g * 0x10001u, p);  // hash = (g << 16) | g
            }
            if constexpr (kHist == HIST_PRIVATE) {
                uint32_t row;
                if constexpr (kLaneBits == 8 && kQMode == QM_FAST16) {
                    const uint32_t d = __umul24(b, p.q_m16) >> 16;
                    row = (uint32_t)__mul24((int)d, neg_q_row) + (b << kRowShift);
                } else {
                    row = queue_of<kQMode>(b, p) << kRowShift;
                }
                lds_add_u64(reinterpret_cast<u64*>(col + row) + k * kBinCols, weight);
            } else if constexpr (kHist == HIST_SHARED) {
                lds_add_u64(&loads[k * p.Q + queue_of<kQMode>(b, p)], weight);
            } else {
                atomicAdd(&rows[(size_t)k * p.q_stride + queue_of<kQMode>(b, p)], weight);
            }
        }
    }
    if constexpr (kHist == HIST_PRIVATE) {
        __syncthreads();
        for (uint32_t e = tid; e < nrows; e += kBlock) {  // e = q * kPat + k
            const uint32_t q = e / kPat, k = e % kPat;
            if (k >= nk) continue;
            const u64 s = row_sum(loads, e);
            if (s) atomicAdd(&rows[(size_t)k * p.q_stride + q], s);
        }
    } else if constexpr (kHist == HIST_SHARED) {
        __syncthreads();
        for (uint32_t e = tid; e < nk * p.Q; e += kBlock) {  // e = k * Q + q
            const uint32_t k = e / p.Q;
            const u64 s = loads[e];
            if (s) atomicAdd(&rows[(size_t)k * p.q_stride + (e - k * p.Q)], s);
        }
    }
}

// ------------------------------------------------------------------- instance picks --
using SymmetricKernelFn = void (*)(const LaunchParams, const u64*, uint32_t);

template <bool kHPow2, int kQMode>
SymmetricKernelFn pick_half_hist(int hist) {
    switch (hist) {
        case HIST_PRIVATE: return rss_symmetric_search_kernel<16, kHPow2, kQMode, HIST_PRIVATE>;
        case HIST_SHARED: return rss_symmetric_search_kernel<16, kHPow2, kQMode, HIST_SHARED>;
        default: return rss_symmetric_search_kernel<16, kHPow2, kQMode, HIST_GLOBAL>;
    }
}

template <bool kHPow2>
SymmetricKernelFn pick_half(int qmode, int hist) {
    switch (qmode) {
        case QM_MASK: return pick_half_hist<kHPow2, QM_MASK>(hist);
        case QM_FAST16: return pick_half_hist<kHPow2, QM_FAST16>(hist);
        default: return pick_half_hist<kHPow2, QM_FAST32>(hist);
    }
}

}  // namespace

// ------------------------------------------------------ launchers (rss_engine.h) --
namespace rss {

int launch_symmetric_fold(const void* d_tuples, uint32_t words, uint32_t fields,
                          const uint32_t* d_weights, size_t n, uint64_t* d_folds, uint32_t flags,
                          hipStream_t stream) {
    if (!(flags & RSS_FLAG_ACCUMULATE)) {
        const int rc = launch_zero_counts(d_folds, RSS_SYMMETRIC_PATTERNS, stream);
        if (rc) return rc;
    }
    if (n == 0) return RSS_OK;
    DeviceInfo info;
    const int rc = device_info(&info);
    if (rc) return rc;
    // addresses are `words - 1` / 2 words each, the ports the two halves of the last word
    FoldMasks m;
    const uint32_t addr_words = (words - 1) / 2;
    for (uint32_t k = 0; k < addr_words; ++k) {
        m.w[k] = fields & RSS_FIELD_SRC_IP ? 0xFFFFFFFFu : 0u;
        m.w[addr_words + k] = fields & RSS_FIELD_DST_IP ? 0xFFFFFFFFu : 0u;
    }
    m.w[words - 1] = (fields & RSS_FIELD_SRC_PORT ? 0xFFFF0000u : 0u) |
                     (fields & RSS_FIELD_DST_PORT ? 0x0000FFFFu : 0u);
    // 128K tuples per workgroup amortise its 16384 bins' clear and flush; every quarter walks
    // all the tuples, so no more than a round of workgroups
    const uint64_t slices = ((uint64_t)n + (1u << 17) - 1) >> 17;
    const unsigned gx = (unsigned)std::min<uint64_t>(slices, std::max(1, info.cu_count / 4));
    auto fn = words == 3 ? rss_symmetric_fold_kernel<3> : rss_symmetric_fold_kernel<9>;
    hipLaunchKernelGGL(fn, dim3(gx, 4), dim3(kBlock), kFoldBinBytes, stream,
                       static_cast<const uint32_t*>(d_tuples), d_weights, (uint64_t)n,
                       reinterpret_cast<u64*>(d_folds), m);
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

// Tier table.  setup_modes sizes u32 bins of one pattern, so it is given an eighth
// of the budget: 4 patterns x Q x 32 x 8 B (or 4 x Q x 8 B shared) fit where Q x 32 x 4 B
// (Q x 4 B) fit an eighth.
int launch_symmetric_search(const uint64_t* d_folds, uint32_t first_pattern, uint32_t npatterns,
                            uint32_t htable, uint32_t nqueues, uint64_t* d_loads,
                            hipStream_t stream) {
    int rc = launch_zero_counts(d_loads, (uint64_t)npatterns * nqueues, stream);
    if (rc) return rc;
    DeviceInfo info;
    rc = device_info(&info);
    if (rc) return rc;
    LaunchParams p;
    memset(&p, 0, sizeof p);
    p.counts = reinterpret_cast<unsigned long long*>(d_loads);
    p.q_stride = nqueues;  // rows keep the caller's nqueues; queues >= min(H, Q) stay zero
    p.nkeys = npatterns;
    const uint32_t q_eff = effective_queues(htable, nqueues, nullptr);
    int qmode, hist;
    uint32_t eighth_bytes;
    const bool h_pow2 = setup_modes(&p, htable, q_eff, true, &qmode, &hist, &eighth_bytes,
                                    kSymBinBytesMax / 8, false);
    const bool bytes = h_pow2 && htable <= 256u &&
                       (uint64_t)q_eff * 8 * kLoadRowBytes <= kSymBinBytesMax;
    const uint32_t per_wg = bytes ? 8 : 4;
    const uint32_t shmem = bytes ? q_eff * 8 * kLoadRowBytes : 8 * eighth_bytes;
    SymmetricKernelFn fn =
        bytes ? (qmode == QM_MASK ? rss_symmetric_search_kernel<8, true, QM_MASK, HIST_PRIVATE>
                                  : rss_symmetric_search_kernel<8, true, QM_FAST16, HIST_PRIVATE>)
              : (h_pow2 ? pick_half<true>(qmode, hist) : pick_half<false>(qmode, hist));
    // the whole range is 8192 or 16384 groups; a few groups split the fold values instead
    const unsigned gy = (npatterns + per_wg - 1) / per_wg;
    unsigned gx = 1;
    while (gx < 64 && 2 * gx * gy <= (unsigned)info.cu_count) gx *= 2;
    hipLaunchKernelGGL(fn, dim3(gx, gy), dim3(kBlock), shmem, stream, p,
                       reinterpret_cast<const u64*>(d_folds), first_pattern);
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

}  // namespace rss
