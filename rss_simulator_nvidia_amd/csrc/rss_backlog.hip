// rss_backlog.hip -- key search by backlog: the deepest each queue's ring gets under each key
// (rss_key_search_backlog_device).  Packets in time order carry a tuple, a tick and a weight (or
// 1); every queue drains `drain` weight units per tick; under key k packet i joins queue q =
// hash_k % H % Q, whose backlog just after it is B = max(B_prev - drain * (tick - tick_prev), 0)
// + w.  d_peaks[key][queue] is the largest B, exact in 64-bit integers.  No test hooks:
// compiled once for both libraries.
//
// Split: two kernels, no workgroup ever waits for another.  The recurrence is sequential in
// time; it is cut into segments of consecutive packets, each reduced on its own to a 4-value
// summary per (segment, key, queue), and a second kernel chains the summaries in order.
//
// Pass 1 (rss_key_search_backlog_kernel).  blockIdx.y is a key group, blockIdx.x a run of S
// consecutive segments.  What bounds this kernel is the scan, one lane per (key, queue) stepping
// through every packet -- not the hashing -- and keys x queues is usually far below the 1024
// lanes (8 keys x 24 queues: 192).  So a workgroup scans S = min(16, 1024 / (keys x q)) segments
// side by side, lane = (segment, key, queue): the idle lanes are put to work by making the cut
// finer, which the chaining allows at any point.  The workgroup walks its segments in rounds of
// c = (1024 / S) & ~3 packets each:
//   hash phase: lane l < S c takes packet l % c of segment l / c, hashes it under all of the
//     group's keys and stages (tick - the segment's first tick, weight) and one queue id per key
//     in LDS slot l; a slot past the segment's end gets the id ~0.  Ids are u8 for q <= 255
//     (~0 must stay free), u16 otherwise.  One packet per lane, dword loads: at ~25 VALU per
//     (lane, packet) of scan the loads are not what the kernel waits for.
//   scan phase: lane (s, k, q) reads segment s's slots four at a time (one ds_read_b128 each
//     for ticks and weights, a b32 / b64 for the ids; the lanes of one (s, k) read one address)
//     and, where the id is q, steps its state -- four 64-bit registers.  With D(t) = drain *
//     (t - t0), t0 the segment's first tick, from G = S = pre = best = 0:
//         G = max(G, D(t)) + w;   best = max(best, G - D(t));
//         S += w;                 pre  = max(pre, S - D(t));
//     G is unsigned (D < 2^63 and a sum of weights < 2^63 need not fit int64 together); G - D,
//     S - D and everything pass 2 forms fit int64 for n < 2^31.
// At the segment's end, with te its last tick, the lane writes best, pre, suf = max(G - D(te),
// 0) and tot = S - D(te); (t0, te) are written once per segment.
// q > 1024 (one key per workgroup, S = 1): a lane owns the queues = its index mod 1024 and the
// states live in LDS (4 x q x 8 B <= 128 KiB), indexed by the id; every lane still reads every
// id, so the scan stays one pass over the round.
//
// Tiers (q = min(H, Q); hashing is the timeline's):
//   packed small tables, power-of-two H <= 256, more than 4 keys, q <= 128: 8 keys per workgroup
//   packed small tables, power-of-two H <= 65536, more than 1 key, q <= 255: 4 keys
//   the single key's small tables, any H: 1 key; q <= 255 u8 ids, q <= 1024 u16 ids, q <= 4096
//     LDS states
//   q > 4096 is refused (kBacklogMaxQueues).
// Keys per workgroup go straight from 4 to 1 rather than by halves: past q = 255 the scan has
// at most 4 lanes' worth of segments to share and the wide pair tables' 120 KiB would take the
// LDS the states need.
//
// Segments.  Their length is n / (S x 2 x CUs / key groups) -- a couple of workgroups per CU --
// at least 256 packets, and never less than n / 8192: at most min(ceil(n / 256), 8192) segments,
// which is what the workspace function promises, whatever the device.
//
// Pass 2 (rss_key_search_backlog_combine_kernel).  One lane per (key, queue column) walks the
// segments in order:
//     xin  = first ? 0 : max(x - drain * (t0 - te_prev), 0)
//     peak = max(peak, best, xin + pre);   x = max(suf, xin + tot)
// and writes d_peaks, the zero columns [q, nqueues) included: no separate clear, and n == 0 is
// this kernel alone.  Nothing is allocated and nothing waits, so the call can be captured.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <algorithm>

#include "rss_engine.h"
#include "rss_kernel_common.h"
#include "rss_keysearch_tables.h"

namespace {

using i64 = long long;

constexpr uint32_t kMaxSegsPerWg = 16;        // S: a segment's round is at least 64 packets
constexpr uint64_t kMinSegPackets = 256;
constexpr uint64_t kMaxSegs = 8192;
constexpr uint32_t kBacklogMaxQueues = 4096;  // q = min(H, Q) served
constexpr uint32_t kCombineBlock = 256;

enum HashKind { HK_PACKED8 = 0, HK_PACKED4 = 1, HK_SINGLE = 2 };

struct BacklogArgs {
    const uint32_t* windows;  // this launch's keys: nkeys x 96 windows
    const uint32_t* tuples;   // n x 3 words
    const uint32_t* weights;  // n, or NULL: 1 per packet
    const uint32_t* ticks;    // n
    uint64_t n;
    uint64_t seg_len;         // packets per segment
    uint64_t h_m64, q_m64;    // ceil(2^64 / H), ceil(2^64 / Q)
    i64* summ;                // [segment][key of the call][queue][best, pre, suf, tot]
    uint32_t* seg_ticks;      // [segment][t0, te]
    uint32_t nseg;
    uint32_t segs_per_wg;     // S
    uint32_t chunk;           // c: packets per segment per round
    uint32_t nkeys;           // in this launch
    uint32_t key0;            // the launch's first key among the call's
    uint32_t nkeys_total;
    uint32_t H, Q;            // Q = min(H, nqueues)
    uint32_t q_m32;           // ceil(2^32 / Q)
    uint32_t drain;
};

struct BacklogState {
    u64 G;
    i64 S, pre, best;
};

// one packet (dt = tick - t0, w) of the lane's queue
__device__ __forceinline__ void backlog_step(BacklogState& s, bool hit, uint32_t dt, uint32_t w,
                                             uint32_t drain) {
    const u64 D = (u64)drain * dt;
    const u64 g = (s.G > D ? s.G : D) + w;
    const i64 sum = s.S + (i64)w;
    if (hit) {
        s.G = g;
        s.S = sum;
        s.best = max(s.best, (i64)(g - D));
        s.pre = max(s.pre, sum - (i64)D);
    }
}

// four consecutive ids from a 4-slot boundary
__device__ __forceinline__ void load_ids(const uint8_t* ids, uint32_t* id) {
    const uint32_t v = *reinterpret_cast<const uint32_t*>(ids);
    id[0] = v & 0xFFu;
    id[1] = (v >> 8) & 0xFFu;
    id[2] = (v >> 16) & 0xFFu;
    id[3] = v >> 24;
}
__device__ __forceinline__ void load_ids(const uint16_t* ids, uint32_t* id) {
    const uint2 v = *reinterpret_cast<const uint2*>(ids);
    id[0] = v.x & 0xFFFFu;
    id[1] = v.x >> 16;
    id[2] = v.y & 0xFFFFu;
    id[3] = v.y >> 16;
}

__device__ __forceinline__ void store_summary(const BacklogArgs& a, uint64_t seg, uint32_t key,
                                              uint32_t q, const BacklogState& s, uint32_t dte) {
    const u64 Dte = (u64)a.drain * dte;
    i64* out = a.summ + ((seg * a.nkeys_total + a.key0 + key) * a.Q + q) * 4;
    out[0] = s.best;
    out[1] = s.pre;
    out[2] = s.G > Dte ? (i64)(s.G - Dte) : 0;
    out[3] = s.S - (i64)Dte;
}

template <int kKind, typename IdT, bool kLdsState>
__global__ __launch_bounds__(kBlock) void rss_key_search_backlog_kernel(const BacklogArgs a) {
    constexpr uint32_t kKeys = kKind == HK_PACKED8 ? 8 : kKind == HK_PACKED4 ? 4 : 1;
    constexpr uint32_t kLaneBits = kKind == HK_PACKED8 ? 8 : 16;
    constexpr uint32_t kNone = (IdT)~0u;
    static_assert(!kLdsState || kKeys == 1, "LDS states: one key per workgroup");
    __shared__ uint2 lut[kPairLutBytes / 8];  // HK_SINGLE: the key's small tables in its front
    __shared__ __align__(16) uint32_t st_dt[kBlock];
    __shared__ __align__(16) uint32_t st_w[kBlock];
    __shared__ __align__(16) IdT st_id[kKeys][kBlock];
    extern __shared__ u64 lds_state[];  // kLdsState: G | S | pre | best, Q each
    const uint32_t tid = threadIdx.x;
    const uint32_t key_first = kKeys * blockIdx.y;
    const uint32_t nvalid = min(kKeys, a.nkeys - key_first);

    if constexpr (kKind == HK_SINGLE) {
        build_small_lut(reinterpret_cast<uint32_t*>(lut),
                        a.windows + (size_t)RSS_INPUT_BITS * key_first, tid);
    } else {
        // lane k of packed[i] = low kLaneBits of key (key_first + k)'s window i (a key past the
        // end repeats the last key; its summaries are not written)
        uint2* packed = reinterpret_cast<uint2*>(st_dt);
        if (tid < RSS_INPUT_BITS) {
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (uint32_t k = 0; k < kKeys; ++k) {
                const uint32_t key = min(key_first + k, a.nkeys - 1);
                const uint32_t w = a.windows[(size_t)RSS_INPUT_BITS * key + tid] &
                                   ((1u << kLaneBits) - 1);
                const uint32_t shift = k * kLaneBits;
                if (shift < 32) lo |= w << shift;
                else hi |= w << (shift - 32);
            }
            packed[tid] = make_uint2(lo, hi);
        }
        __syncthreads();
        build_small_pair_lut(lut, [&](int i) { return packed[i]; }, tid);
    }
    if constexpr (kLdsState)
        for (uint32_t e = tid; e < 4 * a.Q; e += kBlock) lds_state[e] = 0;
    __syncthreads();  // the packed windows are dead: st_dt is staging from here on

    const uint32_t S = a.segs_per_wg, c = a.chunk;
    // hash role: slot tid = packet hj of this workgroup's segment hs
    const uint32_t hs = tid / c, hj = tid % c;
    const uint64_t hseg = (uint64_t)blockIdx.x * S + hs;
    const bool hrole = hs < S && hseg < a.nseg;
    uint64_t hbeg = 0, hend = 0;
    uint32_t ht0 = 0;
    if (hrole) {
        hbeg = hseg * a.seg_len;  // < n: every segment below nseg holds a packet
        hend = min(a.n, hbeg + a.seg_len);
        ht0 = a.ticks[hbeg];
    }
    // scan role: lane (ss, sk, sq), or with LDS states every lane on segment 0
    const uint32_t pairs = kKeys * a.Q;
    const uint32_t ss = kLdsState ? 0u : tid / pairs;
    const uint32_t sk = kLdsState ? 0u : (tid % pairs) / a.Q;
    const uint32_t sq = kLdsState ? 0u : tid % a.Q;  // pairs is a multiple of Q
    const uint64_t sseg = (uint64_t)blockIdx.x * S + ss;
    const bool srole = ss < S && sseg < a.nseg;
    uint64_t slen = 0;
    uint32_t st0 = 0, ste = 0;
    if (srole) {
        const uint64_t sbeg = sseg * a.seg_len;
        const uint64_t send = min(a.n, sbeg + a.seg_len);
        slen = send - sbeg;
        st0 = a.ticks[sbeg];
        ste = a.ticks[send - 1];
    }
    BacklogState reg = {0, 0, 0, 0};
    const uint32_t h_mask = a.H - 1;

    for (uint64_t r0 = 0; r0 < a.seg_len; r0 += c) {  // uniform
        if (tid < S * c) {
            const uint64_t i = hbeg + r0 + hj;
            if (hrole && i < hend) {
                const uint32_t* t = a.tuples + 3 * i;
                const uint32_t w0 = t[0], w1 = t[1], w2 = t[2];
                st_dt[tid] = a.ticks[i] - ht0;
                st_w[tid] = a.weights ? a.weights[i] : 1u;
                if constexpr (kKind == HK_SINGLE) {
                    const uint32_t h = toeplitz_hash_small(reinterpret_cast<const uint32_t*>(lut),
                                                           w0, w1, w2);
                    // Lemire direct remainders, exact for every 32-bit h, H and Q
                    const uint32_t b = (uint32_t)__umul64hi(a.h_m64 * (uint64_t)h, (uint64_t)a.H);
                    st_id[0][tid] = (IdT)__umul64hi(a.q_m64 * (uint64_t)b, (uint64_t)a.Q);
                } else {
                    const uint2 x = toeplitz_hash_pair(lut, w0, w1, w2);
#pragma unroll
                    for (uint32_t k = 0; k < kKeys; ++k) {
                        const uint32_t word = (k * kLaneBits) < 32 ? x.x : x.y;
                        const uint32_t b = (word >> ((k * kLaneBits) & 31)) & h_mask;
                        st_id[k][tid] = (IdT)__umulhi(a.q_m32 * b, a.Q);  // b, Q < 2^16
                    }
                }
            } else {
#pragma unroll
                for (uint32_t k = 0; k < kKeys; ++k) st_id[k][tid] = (IdT)kNone;
            }
        }
        __syncthreads();
        if (srole && slen > r0) {
            const uint32_t cnt = (uint32_t)min((uint64_t)c, slen - r0);
            const uint32_t base = ss * c;  // a multiple of 4
            for (uint32_t j = 0; j < cnt; j += 4) {
                const uint4 dt = *reinterpret_cast<const uint4*>(&st_dt[base + j]);
                const uint4 w = *reinterpret_cast<const uint4*>(&st_w[base + j]);
                uint32_t id[4];
                load_ids(&st_id[sk][base + j], id);
                const uint32_t dts[4] = {dt.x, dt.y, dt.z, dt.w};
                const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    if constexpr (kLdsState) {
                        // the queue's owner: one lane per id, packets in order
                        if (id[e] < a.Q && (id[e] & (kBlock - 1)) == tid) {
                            u64* cell = lds_state + id[e];
                            BacklogState s = {cell[0], (i64)cell[a.Q], (i64)cell[2 * a.Q],
                                              (i64)cell[3 * a.Q]};
                            backlog_step(s, true, dts[e], ws[e], a.drain);
                            cell[0] = s.G;
                            cell[a.Q] = (u64)s.S;
                            cell[2 * a.Q] = (u64)s.pre;
                            cell[3 * a.Q] = (u64)s.best;
                        }
                    } else {
                        backlog_step(reg, id[e] == sq, dts[e], ws[e], a.drain);
                    }
                }
            }
        }
        __syncthreads();
    }

    if (!srole) return;
    if constexpr (kLdsState) {
        for (uint32_t q = tid; q < a.Q; q += kBlock) {
            const u64* cell = lds_state + q;
            const BacklogState s = {cell[0], (i64)cell[a.Q], (i64)cell[2 * a.Q], (i64)cell[3 * a.Q]};
            store_summary(a, sseg, key_first, q, s, ste - st0);
        }
    } else if (sk < nvalid) {
        store_summary(a, sseg, key_first + sk, sq, reg, ste - st0);
    }
    if (blockIdx.y == 0 && sk == 0 && sq == 0 && (!kLdsState || tid == 0)) {
        a.seg_ticks[2 * sseg] = st0;
        a.seg_ticks[2 * sseg + 1] = ste;
    }
}

// pass 2: the segments' summaries chained in time order, one lane per (key, queue column)
__global__ __launch_bounds__(kCombineBlock) void rss_key_search_backlog_combine_kernel(
    const i64* __restrict__ summ, const uint32_t* __restrict__ seg_ticks, uint32_t nseg,
    uint64_t cells, uint32_t nkeys, uint32_t nqueues, uint32_t q_eff, uint32_t drain,
    u64* __restrict__ peaks) {
    const uint64_t idx = (uint64_t)blockIdx.x * kCombineBlock + threadIdx.x;
    if (idx >= cells) return;
    const uint64_t key = idx / nqueues;
    const uint32_t q = (uint32_t)(idx % nqueues);
    if (q >= q_eff) {  // queues no packet can have
        peaks[idx] = 0;
        return;
    }
    const uint64_t stride = (uint64_t)nkeys * q_eff * 4;
    const i64* s = summ + (key * q_eff + q) * 4;
    i64 x = 0, peak = 0;
    uint32_t te_prev = 0;
#pragma unroll 4
    for (uint32_t g = 0; g < nseg; ++g, s += stride) {
        const uint32_t t0 = seg_ticks[2 * g], te = seg_ticks[2 * g + 1];
        const i64 best = s[0], pre = s[1], suf = s[2], tot = s[3];
        const i64 xin = g ? max(x - (i64)((u64)drain * (t0 - te_prev)), (i64)0) : 0;
        peak = max(peak, max(best, xin + pre));
        x = max(suf, xin + tot);
        te_prev = te;
    }
    peaks[idx] = (u64)peak;
}

// ------------------------------------------------------------------------- tiers --
using BacklogKernelFn = void (*)(const BacklogArgs);

struct BacklogTier {
    BacklogKernelFn fn;
    uint32_t keys;       // per workgroup
    uint32_t lds_bytes;  // dynamic: the LDS states
};

// the table in the file header (q_eff <= kBacklogMaxQueues)
inline BacklogTier backlog_tier(uint32_t htable, uint32_t q_eff, size_t nkeys) {
    const bool packed = is_pow2(htable) && htable <= 65536u;
    if (packed && htable <= 256u && nkeys > 4 && q_eff <= 128u)
        return {rss_key_search_backlog_kernel<HK_PACKED8, uint8_t, false>, 8, 0};
    if (packed && nkeys > 1 && q_eff <= 255u)
        return {rss_key_search_backlog_kernel<HK_PACKED4, uint8_t, false>, 4, 0};
    if (q_eff <= 255u) return {rss_key_search_backlog_kernel<HK_SINGLE, uint8_t, false>, 1, 0};
    if (q_eff <= (uint32_t)kBlock)
        return {rss_key_search_backlog_kernel<HK_SINGLE, uint16_t, false>, 1, 0};
    return {rss_key_search_backlog_kernel<HK_SINGLE, uint16_t, true>, 1, q_eff * 32u};
}

inline uint64_t backlog_max_segments(uint64_t n) {
    return std::min<uint64_t>((n + kMinSegPackets - 1) / kMinSegPackets, kMaxSegs);
}

}  // namespace

// ------------------------------------------------------- launcher (rss_engine.h) --
namespace rss {

uint32_t backlog_max_queues() { return kBacklogMaxQueues; }

bool backlog_workspace_bytes(size_t nkeys, size_t n, uint32_t htable, uint32_t nqueues,
                             size_t* out) {
    const uint64_t q_eff = nqueues < htable ? nqueues : htable;
    size_t per_seg = 0, total = 0;
    if (__builtin_mul_overflow(nkeys, (size_t)(q_eff * 32), &per_seg) ||
        __builtin_add_overflow(per_seg, (size_t)8, &per_seg) ||
        __builtin_mul_overflow(per_seg, (size_t)backlog_max_segments(n), &total))
        return false;
    *out = std::max<size_t>(total, 8);
    return true;
}

int launch_search_backlog(const uint32_t* d_windows, size_t nkeys, const rss_tuple4* d_tuples,
                          const uint32_t* d_weights, const uint32_t* d_ticks, size_t n,
                          uint32_t drain, uint32_t htable, uint32_t nqueues, uint64_t* d_peaks,
                          void* d_workspace, hipStream_t stream) {
    const uint32_t q_eff = effective_queues(htable, nqueues, nullptr);
    BacklogArgs a;
    memset(&a, 0, sizeof a);
    if (n) {
        DeviceInfo info;
        int rc = device_info(&info);
        if (rc) return rc;
        const BacklogTier tier = backlog_tier(htable, q_eff, nkeys);
        const size_t max_keys = (size_t)tier.keys * 65535;  // grid.y limit
        const uint64_t key_groups = (std::min(nkeys, max_keys) + tier.keys - 1) / tier.keys;
        a.segs_per_wg = tier.lds_bytes ? 1u
                        : std::min<uint32_t>(kMaxSegsPerWg, kBlock / (tier.keys * q_eff));
        a.chunk = (kBlock / a.segs_per_wg) & ~3u;
        const uint64_t fill = std::max<uint64_t>(1, 2 * (uint64_t)info.cu_count / key_groups);
        const uint64_t want = std::min<uint64_t>(kMaxSegs, a.segs_per_wg * fill);
        a.seg_len = std::max<uint64_t>(kMinSegPackets, (n + want - 1) / want);
        a.nseg = (uint32_t)((n + a.seg_len - 1) / a.seg_len);  // <= backlog_max_segments(n)
        a.tuples = reinterpret_cast<const uint32_t*>(d_tuples);
        a.weights = d_weights;
        a.ticks = d_ticks;
        a.n = n;
        a.H = htable;
        a.Q = q_eff;
        a.h_m64 = magic64(htable);
        a.q_m64 = magic64(q_eff);
        a.q_m32 = magic32(q_eff);
        a.drain = drain;
        a.nkeys_total = (uint32_t)nkeys;
        a.seg_ticks = static_cast<uint32_t*>(d_workspace);
        a.summ = reinterpret_cast<i64*>(a.seg_ticks + 2 * (size_t)a.nseg);
        const unsigned gx = (a.nseg + a.segs_per_wg - 1) / a.segs_per_wg;
        for (size_t k0 = 0; k0 < nkeys; k0 += max_keys) {
            const size_t kn = nkeys - k0 < max_keys ? nkeys - k0 : max_keys;
            a.windows = d_windows + k0 * RSS_INPUT_BITS;
            a.key0 = (uint32_t)k0;
            a.nkeys = (uint32_t)kn;
            hipLaunchKernelGGL(tier.fn, dim3(gx, (unsigned)((kn + tier.keys - 1) / tier.keys)),
                               dim3(kBlock), tier.lds_bytes, stream, a);
            RSS_HIP_CHECK(hipGetLastError());
        }
    }
    const uint64_t cells = (uint64_t)nkeys * nqueues;
    hipLaunchKernelGGL(rss_key_search_backlog_combine_kernel,
                       dim3((unsigned)((cells + kCombineBlock - 1) / kCombineBlock)),
                       dim3(kCombineBlock), 0, stream, a.summ, a.seg_ticks, a.nseg, cells,
                       (uint32_t)nkeys, nqueues, q_eff, drain,
                       reinterpret_cast<u64*>(d_peaks));
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

}  // namespace rss
