// rss_flow_aggregate.hip -- packets to flows on the device (rss_flow_aggregate_device): group n
// tuples of 3 (IPv4) or 9 (IPv6) words by value, sum a u32 weight per group in 64 bits and
// emit the distinct tuples in first-seen order with their loads and first packet indices.
// The step between a capture and the key search's weighted launches.  No test hooks: compiled
// once for both libraries.
//
// Insert-only hash set keyed by reference.  table[cap] (cap = the power of two >= 2n, at least
// kAggMinCap: load <= 0.5) holds packet indices or kEmpty; a slot's tuple is tuples[table[s]],
// immutable input, so a slot is complete the moment its index is visible and nothing is ever
// "being written".  Packet i probes linearly from mix(tuple) & (cap - 1): an empty slot is
// claimed by atomicCAS(kEmpty -> i); an owned slot is compared with tuples[owner] in every
// word -- equal: atomicMin(slot, i) and done, different: next slot.  No lane waits for another
// lane or workgroup: every step is one atomic or one read of immutable data, and the loop is
// bounded by cap.  Slots are never freed and all packets of a flow walk one probe sequence, so a
// flow owns one slot; atomicMin leaves its first packet there whatever the arrival order.
// slot_loads[cap] (u64) takes the weights by one 64-bit atomic add, slot_of[n] the slot of each
// packet.  The result is a function of the input alone: sums of integers and a minimum.
//
// LDS combiner (kCombine).  Traffic is heavy-tailed: a few flows carry most packets, and each
// of them is one table word and one sum that every workgroup's atomics would meet on.  A
// workgroup takes a chunk of kChunk consecutive packets (3072 IPv4, 2048 IPv6: 144 KiB of LDS
// either way), stages their words and weights in LDS through dwordx4 loads (dword loads when
// tuples or weights are not 16-byte aligned, and for the tail), and runs the same claim /
// compare / min on a local table of 2 kChunk slots holding chunk-local indices, with u64
// partial sums (ds_add_u64).  Only the lanes that end up first of their flow in the chunk go to
// the global table, with the chunk's smallest index and summed weight, and leave the global
// slot in an LDS map from which the chunk's other lanes fill slot_of.  Workgroups grid-stride
// over the chunks.  Without kCombine (RSS_AGGREGATE_COMBINER=0, kept for measuring the
// combiner) every packet goes to the global table itself.
//
// Ordered compaction.  Packet i is its flow's first exactly when table[slot_of[i]] == i.  Three
// launches: per-tile (1024 packets) counts of first packets by ballot / popcount, one
// workgroup's scan of the tile counts (it also writes nflows), and the emit pass, which repeats
// the ballot and writes flows, loads and first at tile offset + rank.  No workgroup polls
// another's flag anywhere.
//
// The call clears table and sums with a kernel of its own (no memset node: capturable into a
// graph), so a reused workspace carries nothing over.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <algorithm>

#include "rss_engine.h"
#include "rss_flow_hash.h"
#include "rss_kernel_common.h"
#include "rss_keysearch_tables.h"

namespace {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kAggTile = kBlock;  // packets per compaction tile

template <int kWords>
struct AggChunk {
    // per packet: words + weight staged, 2 local slots x (u32 index + u64 sum + u32 global slot)
    static constexpr uint32_t kChunk = kWords == 3 ? 3072u : 2048u;
    static constexpr uint32_t kSlots = 2 * kChunk;
    static constexpr uint32_t kBytes = kChunk * (kWords + 1) * 4 + kSlots * (4 + 8 + 4);
    static_assert(kChunk % kBlock == 0, "a lane takes kChunk / kBlock packets of a chunk");
    static_assert(kBytes <= kLdsBytes, "the combiner's chunk fits the LDS");
};

struct AggWorkspace {  // views into the caller's workspace
    u64* slot_loads;        // [cap]
    uint32_t* table;        // [cap]
    uint32_t* slot_of;      // [n]
    uint32_t* tile_counts;  // [ntiles]; after the scan the tiles' exclusive offsets
    uint32_t cap;
    uint32_t ntiles;
};

// agg_hash<kWords> (agg_mix, agg_finish): rss_flow_hash.h

template <int kWords>
__device__ __forceinline__ bool agg_equal(const uint32_t* a, const uint32_t* b) {
    uint32_t diff = 0;
#pragma unroll
    for (int k = 0; k < kWords; ++k) diff |= a[k] ^ b[k];
    return diff == 0;
}

// claim / compare / min on table[nslots] for item `idx` whose tuple is `mine`; the tuple of
// index j is rows + kWords * j.  Returns the flow's slot (kEmpty only if every slot belongs to
// another flow, which a load <= 0.5 excludes).  Wait-free: at most nslots probes.
template <int kWords>
__device__ __forceinline__ uint32_t agg_insert(uint32_t* table, uint32_t nslots, uint32_t start,
                                               uint32_t idx, const uint32_t* mine,
                                               const uint32_t* rows) {
    uint32_t s = start;
    for (uint32_t probes = 0; probes < nslots; ++probes) {
        uint32_t owner = __hip_atomic_load(&table[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (owner == kEmpty) {
            owner = atomicCAS(&table[s], kEmpty, idx);
            if (owner == kEmpty) return s;
        }
        if (owner == idx) return s;
        if (agg_equal<kWords>(rows + (size_t)kWords * owner, mine)) {
            if (idx < owner) atomicMin(&table[s], idx);
            return s;
        }
        s = s + 1 == nslots ? 0u : s + 1;
    }
    return kEmpty;
}

// table = kEmpty, sums = 0 (and the flow count, so that n == 0 needs nothing else)
__global__ __launch_bounds__(kBlock) void rss_flow_clear_kernel(const AggWorkspace ws,
                                                                u64* __restrict__ nflows) {
    const uint64_t stride = (uint64_t)gridDim.x * kBlock;
    for (uint64_t e = (uint64_t)blockIdx.x * kBlock + threadIdx.x; e < ws.cap; e += stride) {
        ws.table[e] = kEmpty;
        ws.slot_loads[e] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *nflows = 0;
}

// coalesced copy of `count` dwords src -> LDS dst; dwordx4 when `wide` (src 16-byte aligned)
__device__ __forceinline__ void agg_stage(uint32_t* dst, const uint32_t* __restrict__ src,
                                          uint32_t count, bool wide) {
    uint32_t done = 0;
    if (wide) {
        const uint4* __restrict__ src4 = reinterpret_cast<const uint4*>(src);
        uint4* dst4 = reinterpret_cast<uint4*>(dst);
        for (uint32_t e = threadIdx.x; e < (count >> 2); e += kBlock) dst4[e] = src4[e];
        done = count & ~3u;
    }
    for (uint32_t e = done + threadIdx.x; e < count; e += kBlock) dst[e] = src[e];
}

template <int kWords, bool kCombine>
__global__ __launch_bounds__(kBlock) void rss_flow_insert_kernel(
    const uint32_t* __restrict__ tuples, const uint32_t* __restrict__ weights, const uint64_t n,
    const AggWorkspace ws) {
    const uint32_t tid = threadIdx.x;
    const uint32_t mask = ws.cap - 1;
    if constexpr (kCombine) {
        using C = AggChunk<kWords>;
        constexpr uint32_t kPer = C::kChunk / kBlock;
        __shared__ __attribute__((aligned(16))) uint32_t stage[C::kChunk * kWords];
        __shared__ __attribute__((aligned(16))) uint32_t lweight[C::kChunk];
        __shared__ u64 lsum[C::kSlots];
        __shared__ uint32_t ltable[C::kSlots];
        __shared__ uint32_t lglobal[C::kSlots];  // local slot -> global slot
        static_assert(sizeof stage + sizeof lweight + sizeof lsum + sizeof ltable +
                          sizeof lglobal == C::kBytes, "AggChunk::kBytes is the kernel's LDS");
        // a chunk starts at a multiple of 4 packets: 16-byte alignment is the pointers'
        const bool wide = (((uintptr_t)tuples | (uintptr_t)weights) & 15u) == 0;
        const uint64_t nchunks = (n + C::kChunk - 1) / C::kChunk;
        for (uint64_t chunk = blockIdx.x; chunk < nchunks; chunk += gridDim.x) {
            const uint64_t base = chunk * C::kChunk;
            const uint32_t cnt = (uint32_t)std::min<uint64_t>(C::kChunk, n - base);
            for (uint32_t e = tid; e < C::kSlots; e += kBlock) {
                ltable[e] = kEmpty;
                lsum[e] = 0;
            }
            agg_stage(stage, tuples + base * kWords, cnt * kWords, wide);
            if (weights) agg_stage(lweight, weights + base, cnt, wide);
            __syncthreads();
            uint32_t hash[kPer], lslot[kPer];
#pragma unroll
            for (uint32_t k = 0; k < kPer; ++k) {
                const uint32_t li = tid + k * kBlock;
                if (li >= cnt) continue;
                const uint32_t* mine = stage + li * kWords;
                hash[k] = agg_hash<kWords>(mine);
                // the top bits pick the local slot, the low bits the global one
                lslot[k] = agg_insert<kWords>(ltable, C::kSlots, __umulhi(hash[k], C::kSlots), li,
                                              mine, stage);
                if (lslot[k] != kEmpty)
                    __hip_atomic_fetch_add(&lsum[lslot[k]], (u64)(weights ? lweight[li] : 1u),
                                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kPer; ++k) {  // the chunk's first packet of each flow
                const uint32_t li = tid + k * kBlock;
                if (li >= cnt || lslot[k] == kEmpty || ltable[lslot[k]] != li) continue;
                const uint32_t s = agg_insert<kWords>(ws.table, ws.cap, hash[k] & mask,
                                                      (uint32_t)(base + li), stage + li * kWords,
                                                      tuples);
                if (s != kEmpty) atomicAdd(&ws.slot_loads[s], lsum[lslot[k]]);
                lglobal[lslot[k]] = s;
            }
            __syncthreads();
#pragma unroll
            for (uint32_t k = 0; k < kPer; ++k) {
                const uint32_t li = tid + k * kBlock;
                if (li < cnt) ws.slot_of[base + li] = lslot[k] == kEmpty ? kEmpty : lglobal[lslot[k]];
            }
            // the next chunk's clears touch ltable / lsum / stage, last read before the barrier
            // above; lglobal is next written two barriers on
        }
    } else {
        auto one = [&](uint64_t i, const uint32_t* mine, uint32_t weight) {
            const uint32_t s = agg_insert<kWords>(ws.table, ws.cap, agg_hash<kWords>(mine) & mask,
                                                  (uint32_t)i, mine, tuples);
            if (s != kEmpty) atomicAdd(&ws.slot_loads[s], (u64)weight);
            ws.slot_of[i] = s;
        };
        const uint64_t gtid = (uint64_t)blockIdx.x * kBlock + tid;
        const uint64_t gstride = (uint64_t)gridDim.x * kBlock;
        uint64_t tail_begin = 0;
        if ((((uintptr_t)tuples | (uintptr_t)weights) & 15u) == 0) {  // uniform
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
                for (int t = 0; t < 4; ++t) one(4 * g + t, v + t * kWords, wt[t]);
            }
            tail_begin = ngroups << 2;
        }
        for (uint64_t i = tail_begin + gtid; i < n; i += gstride) {
            uint32_t v[kWords];
#pragma unroll
            for (int k = 0; k < kWords; ++k) v[k] = tuples[kWords * i + k];
            one(i, v, weights ? weights[i] : 1u);
        }
    }
}

// is packet i (of tile * 1024 + tid) its flow's first?  And the lane's rank among the tile's
// first packets, with the tile's total, through one ballot per wave and 16 LDS words.
__device__ __forceinline__ bool agg_is_first(const AggWorkspace& ws, uint64_t i, uint64_t n) {
    if (i >= n) return false;
    const uint32_t s = ws.slot_of[i];
    return s != kEmpty && ws.table[s] == (uint32_t)i;
}

__device__ __forceinline__ uint32_t agg_tile_rank(bool first, uint32_t* wave_counts,
                                                  uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t ballot = __ballot(first);
    if (lane == 0) wave_counts[wave] = (uint32_t)__popcll(ballot);
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kBlock / 64; ++w) {
        const uint32_t c = wave_counts[w];
        before += w < wave ? c : 0u;
        all += c;
    }
    __syncthreads();  // wave_counts is reused by the caller's next tile
    *total = all;
    return before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(kBlock) void rss_flow_count_kernel(const uint64_t n,
                                                                const AggWorkspace ws) {
    __shared__ uint32_t wave_counts[kBlock / 64];
    for (uint32_t tile = blockIdx.x; tile < ws.ntiles; tile += gridDim.x) {
        uint32_t total;
        agg_tile_rank(agg_is_first(ws, (uint64_t)tile * kAggTile + threadIdx.x, n), wave_counts,
                      &total);
        if (threadIdx.x == 0) ws.tile_counts[tile] = total;
    }
}

// one workgroup: tile_counts -> exclusive offsets in place, the total -> nflows.  Lane t owns
// tiles [t * per, (t + 1) * per); the lanes' sums are scanned in LDS.
__global__ __launch_bounds__(kBlock) void rss_flow_scan_kernel(const AggWorkspace ws,
                                                               u64* __restrict__ nflows) {
    __shared__ uint32_t sums[kBlock];
    const uint32_t tid = threadIdx.x;
    const uint32_t per = (ws.ntiles + kBlock - 1) / kBlock;
    const uint32_t begin = std::min(tid * per, ws.ntiles), end = std::min(begin + per, ws.ntiles);
    uint32_t own = 0;
    for (uint32_t t = begin; t < end; ++t) own += ws.tile_counts[t];
    sums[tid] = own;
    __syncthreads();
    for (uint32_t d = 1; d < kBlock; d <<= 1) {  // inclusive scan
        const uint32_t add = tid >= d ? sums[tid - d] : 0u;
        __syncthreads();
        sums[tid] += add;
        __syncthreads();
    }
    uint32_t at = sums[tid] - own;
    for (uint32_t t = begin; t < end; ++t) {
        const uint32_t c = ws.tile_counts[t];
        ws.tile_counts[t] = at;
        at += c;
    }
    if (tid == kBlock - 1) *nflows = sums[tid];
}

template <int kWords>
__global__ __launch_bounds__(kBlock) void rss_flow_emit_kernel(
    const uint32_t* __restrict__ tuples, const uint64_t n, const AggWorkspace ws,
    uint32_t* __restrict__ flows, u64* __restrict__ loads, uint32_t* __restrict__ first) {
    __shared__ uint32_t wave_counts[kBlock / 64];
    for (uint32_t tile = blockIdx.x; tile < ws.ntiles; tile += gridDim.x) {
        const uint64_t i = (uint64_t)tile * kAggTile + threadIdx.x;
        const bool is_first = agg_is_first(ws, i, n);
        uint32_t total;
        const uint32_t rank = agg_tile_rank(is_first, wave_counts, &total);
        if (!is_first) continue;
        const size_t pos = (size_t)ws.tile_counts[tile] + rank;
#pragma unroll
        for (int k = 0; k < kWords; ++k) flows[pos * kWords + k] = tuples[i * kWords + k];
        loads[pos] = ws.slot_loads[ws.slot_of[i]];
        first[pos] = (uint32_t)i;
    }
}

inline size_t round_up8(size_t bytes) { return (bytes + 7) & ~(size_t)7; }

// the table's slots for n packets: the power of two >= 2n, at least kAggMinCap
constexpr uint32_t kAggMinCap = 1024;
inline uint32_t agg_capacity(size_t n) {
    uint32_t cap = kAggMinCap;
    while (cap < 2 * (uint64_t)n) cap <<= 1;  // n <= 2^30: cap <= 2^31
    return cap;
}

}  // namespace

// ------------------------------------------------------ launchers (rss_engine.h) --
namespace rss {

size_t flow_aggregate_workspace_bytes(size_t n) {
    const size_t cap = agg_capacity(n), ntiles = (n + kAggTile - 1) / kAggTile;
    return cap * (sizeof(u64) + sizeof(uint32_t)) + round_up8(n * sizeof(uint32_t)) +
           round_up8(ntiles * sizeof(uint32_t));
}

int launch_flow_aggregate(const void* d_tuples, uint32_t words, const uint32_t* d_weights, size_t n,
                          void* d_flows, uint64_t* d_loads, uint32_t* d_first, uint64_t* d_nflows,
                          void* d_workspace, hipStream_t stream) {
    DeviceInfo info;
    const int rc = device_info(&info);
    if (rc) return rc;
    AggWorkspace ws;
    ws.cap = agg_capacity(n);
    ws.ntiles = (uint32_t)((n + kAggTile - 1) / kAggTile);
    char* at = static_cast<char*>(d_workspace);
    ws.slot_loads = reinterpret_cast<u64*>(at);
    at += (size_t)ws.cap * sizeof(u64);
    ws.table = reinterpret_cast<uint32_t*>(at);
    at += (size_t)ws.cap * sizeof(uint32_t);
    ws.slot_of = reinterpret_cast<uint32_t*>(at);
    at += round_up8(n * sizeof(uint32_t));
    ws.tile_counts = reinterpret_cast<uint32_t*>(at);
    u64* nflows = reinterpret_cast<u64*>(d_nflows);
    const uint32_t* tuples = static_cast<const uint32_t*>(d_tuples);
    const unsigned cus = (unsigned)info.cu_count;
    auto grid = [&](uint64_t units, unsigned per_cu) {
        return dim3((unsigned)std::max<uint64_t>(1, std::min<uint64_t>(units, (uint64_t)per_cu * cus)));
    };

    hipLaunchKernelGGL(rss_flow_clear_kernel, grid((ws.cap + kBlock - 1) / kBlock, 4), dim3(kBlock),
                       0, stream, ws, nflows);
    RSS_HIP_CHECK(hipGetLastError());
    if (n == 0) return RSS_OK;

    const char* env = getenv("RSS_AGGREGATE_COMBINER");
    if (!(env && env[0] == '0')) {
        const uint64_t chunk = words == 3 ? AggChunk<3>::kChunk : AggChunk<9>::kChunk;
        auto fn = words == 3 ? rss_flow_insert_kernel<3, true> : rss_flow_insert_kernel<9, true>;
        hipLaunchKernelGGL(fn, grid((n + chunk - 1) / chunk, 1), dim3(kBlock), 0, stream, tuples,
                           d_weights, (uint64_t)n, ws);
    } else {
        auto fn = words == 3 ? rss_flow_insert_kernel<3, false> : rss_flow_insert_kernel<9, false>;
        hipLaunchKernelGGL(fn, grid((n / 4 + kBlock) / kBlock, 2), dim3(kBlock), 0, stream, tuples,
                           d_weights, (uint64_t)n, ws);
    }
    RSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(rss_flow_count_kernel, grid(ws.ntiles, 8), dim3(kBlock), 0, stream,
                       (uint64_t)n, ws);
    RSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(rss_flow_scan_kernel, dim3(1), dim3(kBlock), 0, stream, ws, nflows);
    RSS_HIP_CHECK(hipGetLastError());
    auto emit = words == 3 ? rss_flow_emit_kernel<3> : rss_flow_emit_kernel<9>;
    hipLaunchKernelGGL(emit, grid(ws.ntiles, 8), dim3(kBlock), 0, stream, tuples, (uint64_t)n, ws,
                       static_cast<uint32_t*>(d_flows), reinterpret_cast<u64*>(d_loads), d_first);
    RSS_HIP_CHECK(hipGetLastError());
    return RSS_OK;
}

}  // namespace rss
