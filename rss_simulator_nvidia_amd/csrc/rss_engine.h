// rss_engine.h -- the engine's launchers (rss_toeplitz.hip, rss_keysearch.hip,
// rss_keysearch6.hip, rss_neighbourhood.hip, rss_byte_neighbourhood.hip,
// rss_keysearch_weighted.hip, rss_timeline.hip, rss_backlog.hip, rss_symmetric.hip,
// rss_flow_aggregate.hip) as the C ABI (rss_host.hip) calls
// them, and the HIP error macro both use.  Internal, not ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rss_internal.h"
#include "rss_toeplitz.h"

// return the failing HIP call as RSS_ENOMEM / RSS_EIO with rss_last_error() set
#define RSS_HIP_CHECK(expr)                                                        \
    do {                                                                           \
        hipError_t e_ = (expr);                                                    \
        if (e_ != hipSuccess)                                                      \
            return rss_set_error(e_ == hipErrorOutOfMemory ? RSS_ENOMEM : RSS_EIO, \
                                 "%s failed: %s", #expr, hipGetErrorString(e_));   \
    } while (0)

namespace rss {

// rss_hash_device[_ws|_reta] on `stream` (reta / ws may be NULL): include/rss_toeplitz.h
RSS_HIDDEN int launch_hash(const rss_key* key, const rss_tuple4* d_tuples, size_t n,
                           uint32_t htable, uint32_t nqueues, uint32_t* d_hash, void* d_queue,
                           uint64_t* d_counts, uint32_t flags, hipStream_t stream,
                           const uint32_t* reta = nullptr, uint64_t* ws = nullptr);
// rss_hash6_device[_ws|_reta]
RSS_HIDDEN int launch_hash6(const rss_key6* key, const rss_tuple6* d_tuples, size_t n,
                            uint32_t htable, uint32_t nqueues, uint32_t* d_hash, void* d_queue,
                            uint64_t* d_counts, uint32_t flags, hipStream_t stream,
                            const uint32_t* reta = nullptr, uint64_t* ws = nullptr);
// rss_key_search_device
RSS_HIDDEN int launch_search(const uint32_t* d_windows, size_t nkeys, const rss_tuple4* d_tuples,
                             size_t n, uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                             hipStream_t stream);
// rss_key_neighbourhood_device (rss_neighbourhood.hip; arguments validated by the caller)
RSS_HIDDEN int launch_neighbourhood(const rss_key* key, const rss_tuple4* d_tuples, size_t n,
                                    uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                                    hipStream_t stream);
// rss_key_search6_device (rss_keysearch6.hip; arguments validated by the caller)
RSS_HIDDEN int launch_search6(const uint32_t* d_windows, size_t nkeys, const rss_tuple6* d_tuples,
                              size_t n, uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                              hipStream_t stream);
// rss_key_neighbourhood6_device (rss_neighbourhood.hip; arguments validated by the caller)
RSS_HIDDEN int launch_neighbourhood6(const rss_key6* key, const rss_tuple6* d_tuples, size_t n,
                                     uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                                     hipStream_t stream);
// rss_key_search_weighted_device / rss_key_neighbourhood_weighted_device
// (rss_keysearch_weighted.hip; arguments validated by the caller)
RSS_HIDDEN int launch_search_weighted(const uint32_t* d_windows, size_t nkeys,
                                      const rss_tuple4* d_tuples, const uint32_t* d_weights,
                                      size_t n, uint32_t htable, uint32_t nqueues,
                                      uint64_t* d_loads, hipStream_t stream);
RSS_HIDDEN int launch_neighbourhood_weighted(const rss_key* key, const rss_tuple4* d_tuples,
                                             const uint32_t* d_weights, size_t n, uint32_t htable,
                                             uint32_t nqueues, uint64_t* d_loads,
                                             hipStream_t stream);
// rss_key_search_timeline_device (rss_timeline.hip; arguments validated by the caller;
// d_weights may be NULL)
RSS_HIDDEN int launch_search_timeline(const uint32_t* d_windows, size_t nkeys,
                                      const rss_tuple4* d_tuples, const uint32_t* d_weights,
                                      const uint32_t* d_slots, size_t n, uint32_t nslots,
                                      uint32_t htable, uint32_t nqueues, uint64_t* d_loads,
                                      hipStream_t stream);
// rss_key_search_backlog_workspace_bytes / rss_key_search_backlog_device (rss_backlog.hip;
// arguments validated by the caller: min(htable, nqueues) <= backlog_max_queues(), the workspace
// 8-byte aligned and large enough; d_weights may be NULL).  backlog_workspace_bytes: false when
// the size overflows size_t.
RSS_HIDDEN uint32_t backlog_max_queues();
RSS_HIDDEN bool backlog_workspace_bytes(size_t nkeys, size_t n, uint32_t htable, uint32_t nqueues,
                                        size_t* out);
RSS_HIDDEN int launch_search_backlog(const uint32_t* d_windows, size_t nkeys,
                                     const rss_tuple4* d_tuples, const uint32_t* d_weights,
                                     const uint32_t* d_ticks, size_t n, uint32_t drain,
                                     uint32_t htable, uint32_t nqueues, uint64_t* d_peaks,
                                     void* d_workspace, hipStream_t stream);
// rss_key_byte_neighbourhood_device / _weighted_device (d_weights non-NULL) / 6_device
// (rss_byte_neighbourhood.hip; arguments validated by the caller)
RSS_HIDDEN int launch_byte_neighbourhood(const rss_key* key, uint32_t first_byte, uint32_t nbytes,
                                         const rss_tuple4* d_tuples, const uint32_t* d_weights,
                                         size_t n, uint32_t htable, uint32_t nqueues,
                                         uint64_t* d_counts, hipStream_t stream);
RSS_HIDDEN int launch_byte_neighbourhood6(const rss_key6* key, uint32_t first_byte,
                                          uint32_t nbytes, const rss_tuple6* d_tuples, size_t n,
                                          uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                                          hipStream_t stream);
// rss_symmetric_fold_device / rss_symmetric_search_device (rss_symmetric.hip; arguments
// validated by the caller)
RSS_HIDDEN int launch_symmetric_fold(const void* d_tuples, uint32_t words, uint32_t fields,
                                     const uint32_t* d_weights, size_t n, uint64_t* d_folds,
                                     uint32_t flags, hipStream_t stream);
RSS_HIDDEN int launch_symmetric_search(const uint64_t* d_folds, uint32_t first_pattern,
                                       uint32_t npatterns, uint32_t htable, uint32_t nqueues,
                                       uint64_t* d_loads, hipStream_t stream);
// rss_flow_aggregate_workspace_bytes / rss_flow_aggregate_device (rss_flow_aggregate.hip;
// arguments validated by the caller, the workspace 8-byte aligned and large enough)
RSS_HIDDEN size_t flow_aggregate_workspace_bytes(size_t n);
RSS_HIDDEN int launch_flow_aggregate(const void* d_tuples, uint32_t words,
                                     const uint32_t* d_weights, size_t n, void* d_flows,
                                     uint64_t* d_loads, uint32_t* d_first, uint64_t* d_nflows,
                                     void* d_workspace, hipStream_t stream);
// d_counts[0, cells) = 0 by a kernel (rss_neighbourhood.hip): capturable, unlike a memset node
RSS_HIDDEN int launch_zero_counts(uint64_t* d_counts, uint64_t cells, hipStream_t stream);
// rss_generate_tuples (n > 0, d_tuples non-NULL)
RSS_HIDDEN int launch_generate(uint64_t seed, uint64_t first_index, size_t n,
                               rss_tuple4* d_tuples, hipStream_t stream);

}  // namespace rss
