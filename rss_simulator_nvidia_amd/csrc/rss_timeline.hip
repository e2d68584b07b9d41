// rss_timeline.hip -- key search over time: the loads each key puts on each queue in each time
// window of a packet stream (rss_key_search_timeline_device).  A packet carries a tuple, a
// weight (or 1) and the window -- the slot -- it falls into; d_loads[key][slot][queue] is the
// exact sum of the weights.  No test hooks: compiled once for both libraries.
//
// Hashing and input are the weighted search's (rss_keysearch_weighted.hip): the packed small
// tables for 8 / 4 keys per ds_read_b64, the wide pair tables for any H, four tuples per lane
// through three dwordx4 loads with a fourth for their weights -- and here a fifth for their
// slots -- when every pointer is 16-byte aligned, else one packet per lane (a uniform branch on
// the pointers).  What is new is the walk and the bins.
//
// Walk.  blockIdx.y is the key group; blockIdx.x owns one contiguous tile of packets, not a
// grid-stride comb, so that on a capture -- packets in time order -- a workgroup meets a short
// run of consecutive slots.  The tile is a multiple of kBlock packets (so it starts on a
// 4-packet group), at least one packet per lane, at most n / (CUs / key groups) -- the tiles
// along x fill the device by themselves, since the typical call scores a handful of keys --
// and, when the slots are not all cached, no longer than (cached - 1) slots of n / nslots
// packets each: the run that traffic of an even rate keeps inside the cache from wherever in
// a slot the tile begins.
//
// Bins.  u64 LDS bins [cached slot][queue][key][32 lane columns]: the 256-byte (queue, key) row
// of the weighted kernels (the 64 banks exactly once, every ds_add_u64 conflict-free, the
// key's offset the immediate), times `cached` slots [s_base, s_base + cached).  s_base is the
// slot of the tile's first packet, lowered where needed so that the range ends at nslots.
// Per packet r = slot - s_base (wrapping): r < cached is one LDS add per key at r's plane; any
// other slot below nslots -- behind s_base or ahead of the range -- is one global 64-bit
// atomic per key; a slot >= nslots is counted nowhere.  Nothing depends on the order of the
// slots but the share of packets that take the atomics.  At the end of the tile each
// non-zero (slot, queue, key) row is one global atomic.  No epochs, no re-basing.
//
// Tiers (q = min(H, Q); S = floor(budget / (q x keys x row)), cached = min(S, nslots)).  Keys
// per workgroup are given up -- halved -- until S >= 2, and first while half of them would
// still hold every key of the call (more slots for the same work):
//   packed tables, power-of-two H <= 65536, budget 158464 B (154.75 KiB), row 256 B
//     8 keys (H <= 256)   q <= 38      S = 3 at q = 24
//     4 keys              q <= 77      S = 6 at q = 24
//     2 keys              q <= 154     S = 12 at q = 24
//     4 keys, shared bins [slot][queue][key] (row 8 B, the columns dropped)   q <= 2476
//   pair tables, any other H, budget 40960 B (40 KiB), 2 keys
//     lane-private, row 256 B   q <= 40
//     shared, row 8 B           q <= 1280
//   past those (packed q > 2476, pair q > 1280): no bins, one global atomic per (packet, key)
//   on the pair tables.
// The pair kernel's tile is at least 32 packets per lane, for its 120 KiB table build.
//
// The loads are cleared by rss_zero_counts_kernel in the same call (n == 0 only clears), so
// the entry can be captured into a graph.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <algorithm>

#include "rss_engine.h"
#include "rss_kernel_common.h"
#include "rss_keysearch_tables.h"

namespace {

// what a timeline launch needs beyond LaunchParams
struct TimelineArgs {
    const uint32_t* weights;  // n, or NULL: 1 per packet
    const uint32_t* slots;    // n
    uint64_t tile;            // packets per workgroup along x (a multiple of kBlock)
    uint32_t nslots;
    uint32_t cached;          // slots in the LDS bins (0: none)
};

using TimelineKernelFn = void (*)(const LaunchParams, const TimelineArgs);

__device__ __forceinline__ void lds_add_load(u64* bin, uint32_t weight) {  // ds_add_u64
    __hip_atomic_fetch_add(bin, (u64)weight, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// first cached slot of this workgroup's tile: its first packet's, with the range kept below
// nslots (cached <= nslots)
__device__ __forceinline__ uint32_t tile_slot_base(const TimelineArgs& a) {
    const uint32_t first = a.slots[(uint64_t)blockIdx.x * a.tile];  // uniform; the tile is not empty
    return min(first, a.nslots - a.cached);
}

// The tile's walk: `count(w0, w1, w2, weight, slot)` for this lane's share of the packets
// [blockIdx.x * tile, min(n, that + tile)).
template <typename Count>
__device__ __forceinline__ void walk_tile(const LaunchParams& p, const TimelineArgs& a, Count count) {
    const uint64_t t0 = (uint64_t)blockIdx.x * a.tile;  // a multiple of 4
    const uint64_t t1 = min(p.n, t0 + a.tile);
    uint64_t tail_begin = t0;
    // a NULL weights pointer adds no bits
    if ((((uintptr_t)p.tuples | (uintptr_t)a.weights | (uintptr_t)a.slots) & 15u) == 0) {  // uniform
        const uint4* __restrict__ src = reinterpret_cast<const uint4*>(p.tuples);
        const uint4* __restrict__ wsrc = reinterpret_cast<const uint4*>(a.weights);
        const uint4* __restrict__ ssrc = reinterpret_cast<const uint4*>(a.slots);
        const uint64_t gend = t1 >> 2;
        for (uint64_t g = (t0 >> 2) + threadIdx.x; g < gend; g += kBlock) {
            const uint4 ta = src[3 * g + 0];
            const uint4 tb = src[3 * g + 1];
            const uint4 tc = src[3 * g + 2];
            const uint4 w = wsrc ? wsrc[g] : make_uint4(1u, 1u, 1u, 1u);
            const uint4 s = ssrc[g];
            count(ta.x, ta.y, ta.z, w.x, s.x);
            count(ta.w, tb.x, tb.y, w.y, s.y);
            count(tb.z, tb.w, tc.x, w.z, s.z);
            count(tc.y, tc.z, tc.w, w.w, s.w);
        }
        tail_begin = gend << 2;  // >= t0
    }
    for (uint64_t i = tail_begin + threadIdx.x; i < t1; i += kBlock) {
        const uint32_t* t = reinterpret_cast<const uint32_t*>(p.tuples) + 3 * i;
        count(t[0], t[1], t[2], a.weights ? a.weights[i] : 1u, a.slots[i]);
    }
}

// loads[key][slot][queue] of this launch's key `key` (p.counts is the launch's first key's)
__device__ __forceinline__ u64* load_cell(const LaunchParams& p, const TimelineArgs& a,
                                          uint32_t key, uint32_t slot, uint32_t q) {
    return p.counts + ((uint64_t)key * a.nslots + slot) * p.q_stride + q;
}

// End of the tile: row e = (r * Q + q) * kKeys + k of the bins -- its 32 columns summed, or
// the shared bin itself -- is one global atomic when it is not zero.
template <uint32_t kKeys, bool kPrivate>
__device__ __forceinline__ void flush_tile(const u64* bins, const LaunchParams& p,
                                           const TimelineArgs& a, uint32_t key0, uint32_t nvalid,
                                           uint32_t s_base) {
    const uint32_t nrows = a.cached * p.Q * kKeys;
    for (uint32_t e = threadIdx.x; e < nrows; e += kBlock) {
        const uint32_t k = e % kKeys, rq = e / kKeys;
        if (k >= nvalid) continue;
        const u64 s = kPrivate ? row_sum(bins, e) : bins[e];
        if (s) atomicAdd(load_cell(p, a, key0 + k, s_base + rq / p.Q, rq % p.Q), s);
    }
}

// ------------------------------------------------------------------ packed tables --
// kKeys keys per workgroup on the 21 conflict-free ds_read_b64 of the packed search kernel:
// byte lanes (kLaneBits 8: 8 keys, H <= 256) or half-word lanes (16: 4 or 2 keys, H <= 65536).
// Bins u64 [slot][queue][key][column] (kHist HIST_PRIVATE) or [slot][queue][key] (HIST_SHARED).
template <int kLaneBits, uint32_t kKeys, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_key_search_timeline_packed_kernel(
    const LaunchParams p, const TimelineArgs a) {
    static_assert(kKeys * kLaneBits <= 64 && (kKeys & (kKeys - 1)) == 0, "keys fit the 64-bit entry");
    constexpr bool kPrivate = kHist == HIST_PRIVATE;
    constexpr uint32_t kRowBytes = kPrivate ? kLoadRowBytes : 8u;       // one (queue, key)
    constexpr uint32_t kQueueBytes = kKeys * kRowBytes;                 // one queue's keys
    __shared__ uint2 lut[kPairLutBytes / 8];
    extern __shared__ u64 loads[];
    const uint32_t tid = threadIdx.x;
    const uint32_t key0 = kKeys * blockIdx.y;
    const uint32_t nvalid = min(kKeys, p.nkeys - key0);

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
    const uint32_t slot_bytes = p.Q * kQueueBytes;  // one cached slot's plane
    for (uint32_t e = tid; e < a.cached * (slot_bytes / 8); e += kBlock) loads[e] = 0;
    __syncthreads();

    const uint32_t s_base = tile_slot_base(a);
    char* col = reinterpret_cast<char*>(loads + (kPrivate ? tid & (kBinCols - 1) : 0u));
    const uint32_t hbits = 31 - __clz(p.H);  // log2(H)
    // byte lanes: q * kQueueBytes = b * kQueueBytes - d * (Q * kQueueBytes), d = floor(b / Q):
    // two full-rate 24-bit multiplies (Q <= 38 rows of 2 KiB and b < 256 fit 24 bits)
    const int neg_q_row = -(int)slot_bytes;
    const uint32_t lane_mask4 = (p.H - 1) * 0x01010101u;
    walk_tile(p, a, [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t weight, uint32_t slot) {
        uint2 x = toeplitz_hash_pair(lut, w0, w1, w2);
        if constexpr (kLaneBits == 8) {
            x.x &= lane_mask4;
            x.y &= lane_mask4;
        }
        const uint32_t r = slot - s_base;  // wraps for a slot behind the range
        const bool in_lds = r < a.cached;
        if (!in_lds && slot >= a.nslots) return;
        char* plane = col + (in_lds ? r * slot_bytes : 0u);
#pragma unroll
        for (uint32_t k = 0; k < kKeys; ++k) {
            const uint32_t word = (k * kLaneBits) < 32 ? x.x : x.y;
            const uint32_t b = kLaneBits == 8 ? (word >> ((k * 8) & 31)) & 0xFFu
                                              : __builtin_amdgcn_ubfe(word, (k * kLaneBits) & 31, hbits);
            if (in_lds) {
                uint32_t row;
                if constexpr (kLaneBits == 8 && kQMode == QM_FAST16) {
                    const uint32_t d = __umul24(b, p.q_m16) >> 16;
                    row = (uint32_t)__mul24((int)d, neg_q_row) + b * kQueueBytes;
                } else {
                    row = queue_of<kQMode>(b, p) * kQueueBytes;
                }
                lds_add_load(reinterpret_cast<u64*>(plane + row + k * kRowBytes), weight);
            } else if (k < nvalid) {
                atomicAdd(load_cell(p, a, key0 + k, slot, queue_of<kQMode>(b, p)), (u64)weight);
            }
        }
    });
    __syncthreads();
    flush_tile<kKeys, kPrivate>(loads, p, a, key0, nvalid, s_base);
}

// -------------------------------------------------------------------- pair tables --
// Any H: keys 2y and 2y + 1 on the nine wide tables (two full hashes per packet); bins u64
// [slot][queue][key][column] (private), [slot][queue][key] (shared) or none (global atomics).
template <bool kHPow2, int kQMode, int kHist>
__global__ __launch_bounds__(kBlock) void rss_key_search_timeline_pair_kernel(
    const LaunchParams p, const TimelineArgs a) {
    constexpr bool kPrivate = kHist == HIST_PRIVATE;
    constexpr uint32_t kRowCells = kPrivate ? kBinCols : 1u;  // u64 per (queue, key)
    __shared__ uint2 lut[kWidePairLutBytes / 8];
    extern __shared__ u64 loads[];
    const uint32_t tid = threadIdx.x;
    // an odd last key is paired with itself and its copy neither flushed nor added
    const uint32_t key_a = 2 * blockIdx.y;
    const uint32_t nvalid = min(2u, p.nkeys - key_a);
    const uint32_t key_b = key_a + nvalid - 1;
    build_wide_pair_lut(lut, p.key_windows + (size_t)RSS_INPUT_BITS * key_a,
                        p.key_windows + (size_t)RSS_INPUT_BITS * key_b, tid);
    const uint32_t slot_cells = kHist == HIST_GLOBAL ? 0u : p.Q * 2 * kRowCells;
    for (uint32_t e = tid; e < a.cached * slot_cells; e += kBlock) loads[e] = 0;
    __syncthreads();

    const uint32_t s_base = kHist == HIST_GLOBAL ? 0u : tile_slot_base(a);
    u64* col = loads + (kPrivate ? tid & (kBinCols - 1) : 0u);
    uint32_t hi = 65536u;
    asm volatile("" : "+v"(hi));
    walk_tile(p, a, [&](uint32_t w0, uint32_t w1, uint32_t w2, uint32_t weight, uint32_t slot) {
        const uint2 h = toeplitz_hash_wide_pair(lut, w0, w1, w2, hi);
        const uint32_t qa = queue_of<kQMode>(bucket_of<kHPow2>(h.x, p), p);
        const uint32_t qb = queue_of<kQMode>(bucket_of<kHPow2>(h.y, p), p);
        const uint32_t r = slot - s_base;  // wraps for a slot behind the range
        if (kHist != HIST_GLOBAL && r < a.cached) {
            u64* plane = col + r * slot_cells;
            lds_add_load(plane + (qa * 2 + 0) * kRowCells, weight);
            lds_add_load(plane + (qb * 2 + 1) * kRowCells, weight);
        } else if (slot < a.nslots) {
            atomicAdd(load_cell(p, a, key_a, slot, qa), (u64)weight);
            if (nvalid == 2) atomicAdd(load_cell(p, a, key_b, slot, qb), (u64)weight);
        }
    });
    if constexpr (kHist != HIST_GLOBAL) {
        __syncthreads();
        flush_tile<2, kPrivate>(loads, p, a, key_a, nvalid, s_base);
    }
}

// ------------------------------------------------------------------- instance picks --
template <int kLaneBits, uint32_t kKeys, int kHist>
TimelineKernelFn pick_packed_qmode(int qmode) {
    return qmode == QM_MASK ? rss_key_search_timeline_packed_kernel<kLaneBits, kKeys, QM_MASK, kHist>
                            : rss_key_search_timeline_packed_kernel<kLaneBits, kKeys, QM_FAST16, kHist>;
}

TimelineKernelFn pick_packed(uint32_t keys, int hist, int qmode) {
    if (hist == HIST_SHARED) return pick_packed_qmode<16, 4, HIST_SHARED>(qmode);
    switch (keys) {
        case 8: return pick_packed_qmode<8, 8, HIST_PRIVATE>(qmode);
        case 4: return pick_packed_qmode<16, 4, HIST_PRIVATE>(qmode);
        default: return pick_packed_qmode<16, 2, HIST_PRIVATE>(qmode);
    }
}

template <bool kHPow2, int kQMode>
TimelineKernelFn pick_pair_hist(int hist) {
    switch (hist) {
        case HIST_PRIVATE: return rss_key_search_timeline_pair_kernel<kHPow2, kQMode, HIST_PRIVATE>;
        case HIST_SHARED: return rss_key_search_timeline_pair_kernel<kHPow2, kQMode, HIST_SHARED>;
        default: return rss_key_search_timeline_pair_kernel<kHPow2, kQMode, HIST_GLOBAL>;
    }
}

template <bool kHPow2>
TimelineKernelFn pick_pair(int qmode, int hist) {
    switch (qmode) {
        case QM_MASK: return pick_pair_hist<kHPow2, QM_MASK>(hist);
        case QM_FAST16: return pick_pair_hist<kHPow2, QM_FAST16>(hist);
        default: return pick_pair_hist<kHPow2, QM_FAST32>(hist);
    }
}

// ------------------------------------------------------------------------- tiers --
struct TimelineTier {
    bool packed;     // packed small tables (else the wide pair tables)
    int hist;        // HIST_PRIVATE / HIST_SHARED / HIST_GLOBAL
    uint32_t keys;   // per workgroup
    uint32_t slots;  // S: slots whose bins fit (0 for HIST_GLOBAL)
};

constexpr uint32_t kMinCachedSlots = 2;  // fewer and a tile's second window is all atomics

inline uint32_t slots_that_fit(uint32_t budget, uint32_t q_eff, uint32_t keys, uint32_t row_bytes) {
    return (uint32_t)(budget / ((uint64_t)q_eff * keys * row_bytes));
}

// the table in the file header
inline TimelineTier timeline_tier(uint32_t htable, uint32_t q_eff, size_t nkeys) {
    if (is_pow2(htable) && htable <= 65536u) {
        uint32_t keys = htable <= 256u ? 8 : 4;
        while (keys > 2 && keys / 2 >= nkeys) keys /= 2;  // fewer bins per slot, the same work
        while (keys > 2 && slots_that_fit(kPackedBinBytesMax, q_eff, keys, kLoadRowBytes) < kMinCachedSlots)
            keys /= 2;
        uint32_t s = slots_that_fit(kPackedBinBytesMax, q_eff, keys, kLoadRowBytes);
        if (s >= kMinCachedSlots) return {true, HIST_PRIVATE, keys, s};
        s = slots_that_fit(kPackedBinBytesMax, q_eff, 4, 8);
        if (s >= kMinCachedSlots) return {true, HIST_SHARED, 4, s};
        return {false, HIST_GLOBAL, 2, 0};
    }
    uint32_t s = slots_that_fit(kWidePairBinBytesMax, q_eff, 2, kLoadRowBytes);
    if (s >= kMinCachedSlots) return {false, HIST_PRIVATE, 2, s};
    s = slots_that_fit(kWidePairBinBytesMax, q_eff, 2, 8);
    if (s >= kMinCachedSlots) return {false, HIST_SHARED, 2, s};
    return {false, HIST_GLOBAL, 2, 0};
}

// Packets per workgroup along x (file header, "Walk"): a multiple of kBlock.
inline uint64_t timeline_tile(uint64_t n, uint32_t nslots, uint32_t cached, bool packed,
                              uint64_t key_groups, int cu_count) {
    const uint64_t fill = std::max<uint64_t>(1, (uint64_t)cu_count / key_groups);
    uint64_t tile = (n + fill - 1) / fill;
    if (cached && cached < nslots) {
        const uint64_t per_slot = (n + nslots - 1) / nslots;
        tile = std::min(tile, (uint64_t)(cached - 1) * per_slot);
    }
    tile = std::max<uint64_t>(tile, (packed ? 1 : 32) * (uint64_t)kBlock);
    tile = std::max<uint64_t>(tile, (n + (1u << 30) - 1) >> 30);  // gridDim.x stays below 2^31
    return (tile + kBlock - 1) / kBlock * kBlock;
}

}  // namespace

// ------------------------------------------------------- launcher (rss_engine.h) --
namespace rss {

int launch_search_timeline(const uint32_t* d_windows, size_t nkeys, const rss_tuple4* d_tuples,
                           const uint32_t* d_weights, const uint32_t* d_slots, size_t n,
                           uint32_t nslots, uint32_t htable, uint32_t nqueues, uint64_t* d_loads,
                           hipStream_t stream) {
    static_assert(kBlock % 4 == 0, "a tile starts on a 4-packet group");
    int rc = launch_zero_counts(d_loads, (uint64_t)nkeys * nslots * nqueues, stream);
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
    int qmode, hist_unused;
    uint32_t bytes_unused;
    const bool h_pow2 = setup_modes(&p, htable, q_eff, true, &qmode, &hist_unused, &bytes_unused,
                                    kWidePairBinBytesMax, false);
    const TimelineTier tier = timeline_tier(htable, q_eff, nkeys);
    TimelineArgs a;
    a.weights = d_weights;
    a.slots = d_slots;
    a.nslots = nslots;
    a.cached = std::min(tier.slots, nslots);
    const uint32_t row_bytes = tier.hist == HIST_PRIVATE ? kLoadRowBytes : 8u;
    const uint32_t bin_bytes = a.cached * q_eff * tier.keys * row_bytes;  // <= the tier's budget
    const uint32_t shmem = tier.packed ? std::max(bin_bytes, kPackedPrepBytes) : bin_bytes;
    TimelineKernelFn fn = tier.packed ? pick_packed(tier.keys, tier.hist, qmode)
                          : h_pow2    ? pick_pair<true>(qmode, tier.hist)
                                      : pick_pair<false>(qmode, tier.hist);
    const size_t max_keys = (size_t)tier.keys * 65535;  // grid.y limit
    const uint64_t key_groups = (std::min(nkeys, max_keys) + tier.keys - 1) / tier.keys;
    a.tile = timeline_tile(n, nslots, a.cached, tier.packed, key_groups, info.cu_count);
    const unsigned gx = (unsigned)((n + a.tile - 1) / a.tile);
    for (size_t k0 = 0; k0 < nkeys; k0 += max_keys) {
        const size_t kn = nkeys - k0 < max_keys ? nkeys - k0 : max_keys;
        p.key_windows = d_windows + k0 * RSS_INPUT_BITS;
        p.counts = reinterpret_cast<unsigned long long*>(d_loads + k0 * (uint64_t)nslots * nqueues);
        p.nkeys = (uint32_t)kn;
        hipLaunchKernelGGL(fn, dim3(gx, (unsigned)((kn + tier.keys - 1) / tier.keys)), dim3(kBlock),
                           shmem, stream, p, a);
        RSS_HIP_CHECK(hipGetLastError());
    }
    return RSS_OK;
}

}  // namespace rss
