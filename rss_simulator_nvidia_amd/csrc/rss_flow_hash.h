// rss_flow_hash.h -- the hash of the flow table in rss_flow_aggregate.hip: a chain of bijections
// on 32 bits (xor a word, multiply by an odd constant, rotate; murmur3's finaliser), so a tuple
// with any chosen hash exists for any choice of its other words.  The top bits pick the slot of
// the combiner's local table, the low bits the global one.  Host and device: tests/flow_hash.py
// is its numpy port and tests/native/flow_hash_main.cpp compiles this file alone to check it.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define RSS_FLOW_HASH_FN __host__ __device__ __forceinline__
#else
#define RSS_FLOW_HASH_FN inline
#endif

RSS_FLOW_HASH_FN uint32_t agg_mix(uint32_t h, uint32_t w) {
    h = (h ^ w) * 0x9E3779B1u;
    return (h << 15) | (h >> 17);
}

RSS_FLOW_HASH_FN uint32_t agg_finish(uint32_t h) {  // murmur3's finaliser
    h ^= h >> 16;
    h *= 0x85EBCA6Bu;
    h ^= h >> 13;
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

template <int kWords>
RSS_FLOW_HASH_FN uint32_t agg_hash(const uint32_t* t) {
    uint32_t h = 0x2545F491u;
#pragma unroll
    for (int k = 0; k < kWords; ++k) h = agg_mix(h, t[k]);
    return agg_finish(h);
}
