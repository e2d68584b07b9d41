/*
 * rss_toeplitz.h -- C ABI of the MI355X (gfx950) RSS Toeplitz hashing engine.
 *
 * This is the drop-in boundary for the reference's hot path.  The reference
 * (noamsto/rss_simulator_nvidia v0.0.2) is pure Python and has no FFI, so each
 * entry point below names the Python function whose job it takes over; the
 * Python mirror in rss_simulator_nvidia_amd/ binds them through ctypes
 * (rss_simulator_nvidia_amd/_native.py) and INTEGRATION.md shows the ctypes stub
 * a reference maintainer would add.
 *
 * Conventions
 *   - plain C types only; buffers are caller-owned; nothing here allocates on
 *     behalf of the caller except an rss_ctx (which owns its device scratch);
 *   - every function returns RSS_OK (0) or a negative errno-style code and never
 *     aborts; rss_last_error() returns a thread-local message for the last
 *     failure on the calling thread;
 *   - "device" entry points take device pointers and a hipStream_t passed as
 *     void* (NULL = the legacy default stream) and are stream-ordered: they
 *     enqueue work and return without synchronising;
 *   - all arithmetic is integer and bit-exact to the reference.
 */
#ifndef RSS_TOEPLITZ_H
#define RSS_TOEPLITZ_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSS_ABI_VERSION 2

/* status codes (negative errno values) */
#define RSS_OK 0
#define RSS_EIO (-5)      /* HIP runtime / device failure                         */
#define RSS_ENOMEM (-12)  /* device or pinned allocation failed                   */
#define RSS_EINVAL (-22)  /* bad argument (NULL, bad key length, zero htable ...) */
#define RSS_ENODEV (-19)  /* no usable gfx950 device                              */
#define RSS_ENOTSUP (-95) /* CSV not in the canonical fast-path form (use pandas)  */

/*
 * One IPv4 4-tuple, packed to 12 bytes, 4-byte aligned.  The three host-order
 * words are exactly the 96-bit big-endian Toeplitz input of
 * rss_simulator/toeplitz.py:113-142 (__prepare_input_bytes): src_ip, dst_ip,
 * then (src_port & 0xFFFF) << 16 | (dst_port & 0xFFFF).  Ports are masked to 16
 * bits by the caller, matching toeplitz.py:138-141.
 */
typedef struct rss_tuple4 {
    uint32_t sip;
    uint32_t dip;
    uint32_t ports;
} rss_tuple4;

#define RSS_KEY_MIN_BYTES 4
#define RSS_KEY_MAX_BYTES 52
#define RSS_INPUT_BITS 96

/*
 * Prepared hash key.  window[i] is the 32-bit window the reference XORs in
 * for input bit i (toeplitz.py:65-68 with __key_left_most_32bits :71-81 after i
 * rotations by __shift_key :83-98), i.e. key bits [i, i+32) MSB-first (bit
 * indices taken modulo 8*len, which only matters for keys shorter than 16
 * bytes).  The device kernel expands the windows into its LDS lookup tables.
 * For len >= 16 only key bytes 0..15 influence any hash.
 */
typedef struct rss_key {
    uint32_t len;                          /* key length in bytes (>= 4)     */
    uint8_t bytes[RSS_KEY_MAX_BYTES];      /* first min(len, 52) key bytes   */
    uint32_t window[RSS_INPUT_BITS];
} rss_key;

/*
 * Replaces HashKey.__from_str's conversion result -> Toeplitz(key)
 * (rss_simulator/hash_key.py:12-32, rss_simulator/toeplitz.py:8-15).  `key`
 * holds `len` raw bytes, len >= 4.  The CLI's key regex admits only 40 or 52
 * (hash_key.py:25-28), but Toeplitz(list) accepts any list of >= 4 bytes, and a
 * key shorter than 16 bytes wraps during the rotation -- reproduced here.  Text
 * parsing stays in the caller.
 */
int rss_key_prepare(const uint8_t* key, size_t len, rss_key* out);

/*
 * Field selection (the reference's planned "select what
 * will be the fields used for the RSS function", docs/rss_general_explaination.md:14-18,
 * i.e. ethtool's rx-flow-hash s/d/f/n).  The hash input becomes the concatenation
 * of the selected fields in the order src_ip, dst_ip, src_port, dst_port.  Since
 * Toeplitz is linear in the input bits, that equals hashing the full 12-byte tuple
 * with window[i] replaced by the window of bit i's position in the concatenation
 * (0 for unselected bits): the kernel is unchanged.  Apply once, after
 * rss_key_prepare.  RSS_FIELDS_IP is the "IPv4 only" hash of the Microsoft RSS
 * verification suite.
 */
#define RSS_FIELD_SRC_IP 1u
#define RSS_FIELD_DST_IP 2u
#define RSS_FIELD_SRC_PORT 4u
#define RSS_FIELD_DST_PORT 8u
#define RSS_FIELDS_IP (RSS_FIELD_SRC_IP | RSS_FIELD_DST_IP)
#define RSS_FIELDS_ALL 15u
int rss_key_select_fields(rss_key* key, uint32_t fields);

/* flags for rss_hash_device / rss_hash_host */
#define RSS_FLAG_ACCUMULATE 1u  /* add into counts instead of overwriting them      */
#define RSS_FLAG_QUEUE_U16 2u   /* rss_hash_device: d_queue is uint16_t[n] (Q<=2^16) */
#define RSS_FLAG_QUEUE_U8 4u    /* rss_hash_device: d_queue is uint8_t[n]  (Q<=256)  */
/* rss_hash_device: 64-bit addressing even where every stream's byte offsets fit 32 bits
 * (the instance batches of >= 2^32 / 12 tuples run).  Same results and the same access
 * shape; it only gives the launch a kernel symbol of its own in traces -- the placement
 * probe and the clock settle use it, so a profile's row for the 32-bit instance holds the
 * resident step's launches alone. */
#define RSS_FLAG_ADDR64 8u

/*
 * Device-resident hot path.  Replaces, for n tuples at once:
 *   Simulator.calc_hash          rss_simulator/simulator.py:74-92
 *     -> Toeplitz.compute_hash    rss_simulator/toeplitz.py:46-69
 *   Simulator.calc_queue_number  rss_simulator/simulator.py:94-98
 *     (queue = hash % htable % nqueues)
 *   the value_counts of Simulator.write_statistics  simulator.py:107-113
 *     (counts[q] = number of tuples with queue q, for q < nqueues).
 * d_tuples: n packed tuples in device memory.  d_hash: n uint32 or NULL.
 * d_queue: n queue numbers or NULL -- uint32 by default, uint16 / uint8 with
 * RSS_FLAG_QUEUE_U16 / RSS_FLAG_QUEUE_U8 (same values, narrower stores; the flag is
 * rejected if the queues do not fit).  Every queue is < min(htable, nqueues) (bucket <
 * htable), so bins, the width check and the counts the kernel writes are sized by
 * min(htable, nqueues): --num-queues 4e9 with htable 128 fits a u8 column and 128 bins.
 * d_counts: nqueues uint64 or NULL; overwritten unless RSS_FLAG_ACCUMULATE (entries
 * [min(htable, nqueues), nqueues) are then zero -- callers may size counts by
 * min(htable, nqueues) and pass that as nqueues).  htable >= 1, nqueues >= 1
 * (positive_int.py:27).  Launched on `stream` (hipStream_t) on the calling
 * thread's current device.  Any alignment works; 16-byte aligned tuples/hashes
 * (and 4/8/16-byte aligned u8/u16/u32 queues) take the 4-tuples-per-lane path.
 * Counts-only launches with a power-of-two htable <= 256 run a table-free kernel;
 * with more than 8192 queues the counts go to guarded LDS bins of the hash pass itself --
 * u16 bins for up to 16384 queues beside the 12-bit tables and up to 80572 beside the
 * 2.6 KiB small tables (4-tuple body, no indirection table), u8 bins for up to 161144 --
 * whose per-workgroup rows a reduce launch sums; the queues past that are counted by wide
 * passes (163840 queues per pass in u8 bins, 65536 in u16) over d_queue when given, else --
 * counts only -- over per-wave lists of the tuples whose queue lies past the LDS range (the
 * queue minus 161144, 2 bytes per entry for nqueues <= 226680, else 4).  A guarded bin that
 * wraps (a batch piling many tuples onto one queue at once) poisons its pass and a gated
 * recount with u32 bins replaces that pass's counts: exact for any input.  Scratch for the
 * rows, the lists and the passes is stream-ordered hipMallocAsync / hipFreeAsync on
 * `stream`, all of it taken before the first pass touches d_counts; a launch that cannot
 * get it counts with one global atomic per tuple instead (same counts, slower), as it does
 * when a guarded path would need more narrow passes than the atomics cost.
 */
int rss_hash_device(const rss_key* key, const rss_tuple4* d_tuples, size_t n,
                    uint32_t htable, uint32_t nqueues, uint32_t* d_hash,
                    void* d_queue, uint64_t* d_counts, uint32_t flags,
                    void* stream);

/*
 * Single-pass counts: rss_hash_device with a caller-owned workspace, so that a batch's
 * counts need no zeroing launch before it (the step of a job that hashes batch after
 * batch into fresh counts, sharding.CountsPipeline).  Every workgroup adds, for every
 * queue, its bin total plus one arrival (1 << 44) into the workspace; the add that sees the
 * last arrival writes that queue's count into d_counts -- overwriting it, or adding with
 * RSS_FLAG_ACCUMULATE -- and zeroes its word again.  d_workspace: rss_counts_workspace_bytes(nqueues) bytes of 8-byte
 * aligned device memory (one word per queue + the balanced tail's unit counter + one spare),
 * zero before its first use (every launch leaves it zero), used
 * by one launch at a time (launches that may run concurrently need their own).  Launches
 * whose counts are not gathered in private/shared LDS bins (more than 8192 queues) leave the workspace
 * untouched and zero d_counts first as rss_hash_device does.  Results are identical to
 * rss_hash_device's.  With d_counts NULL the workspace is not used (may be NULL).
 * Ordering: a queue's count travels in the atomics on its own word, and the balanced
 * tail's counter (below) is reset by the launch's final claim on it, so no fence is needed
 * (the memory model's single-location coherence); stress-tested in
 * tests/test_gpu_single_pass.py.  Launches of >= 2^24 tuples
 * also take the last tenth of their work from a counter in the workspace (the balanced tail: the XCDs finish
 * together), so a workspace must never be shared by two launches in flight.
 */
int rss_counts_workspace_bytes(uint32_t nqueues, size_t* out);
int rss_hash_device_ws(const rss_key* key, const rss_tuple4* d_tuples, size_t n,
                       uint32_t htable, uint32_t nqueues, uint32_t* d_hash,
                       void* d_queue, uint64_t* d_counts, uint32_t flags,
                       uint64_t* d_workspace, void* stream);

/*
 * Indirection table (RETA; `ethtool -X equal N / weight ...`, which the reference's
 * docs cite, docs/rss_general_explaination.md:9-11): queue = reta[hash % htable]
 * instead of (hash % htable) % nqueues.  reta: host array of htable entries, each
 * < nqueues; htable <= 1024.  The reference's mapping is the table reta[b] = b %
 * nqueues ("equal").  Everything else as rss_hash_device / rss_hash_host.
 */
int rss_hash_device_reta(const rss_key* key, const rss_tuple4* d_tuples, size_t n,
                         uint32_t htable, const uint32_t* reta, uint32_t nqueues,
                         uint32_t* d_hash, void* d_queue, uint64_t* d_counts, uint32_t flags,
                         void* stream);

/*
 * Synthetic input: tuple i (i = first_index .. first_index+n-1) is
 *   r0 = mix64(seed + 2i), r1 = mix64(seed + 2i + 1)       (mod 2^64)
 *   sip = r0 >> 32, dip = (uint32)r0, ports = (uint32)r1
 * with mix64 the splitmix64 finaliser (gamma 0x9E3779B97F4A7C15).  The oracle
 * restates the same generator, so any shard can be rebuilt on the host.
 */
int rss_generate_tuples(uint64_t seed, uint64_t first_index, size_t n,
                        rss_tuple4* d_tuples, void* stream);

/*
 * Key search (the reference's random_hash_key,
 * hash_key.py:53-60, is the candidate generator this evaluates at scale): for
 * each of nkeys keys, the per-queue counts of the same n device-resident tuples.
 * d_windows: nkeys x 96 uint32 in device memory, key k's rss_key::window at
 * k*96.  d_counts: nkeys x nqueues uint64, row k = key k, overwritten.  One
 * launch; each workgroup builds one key's tables and histograms a slice.
 */
int rss_key_search_device(const uint32_t* d_windows, size_t nkeys,
                          const rss_tuple4* d_tuples, size_t n, uint32_t htable,
                          uint32_t nqueues, uint64_t* d_counts, void* stream);

/*
 * A key's single-bit-flip neighbourhood (key search's local step; keysearch.refine climbs
 * on it): the per-queue counts of the same n device-resident tuples under each of the
 * RSS_KEY_NEIGHBOURS keys that differ from `key` in one bit.  Neighbour j has key bit j
 * flipped (bit 0 = MSB of byte 0: byte j >> 3, mask 0x80 >> (j & 7)); these 128 bits are the
 * ones of bytes 0..15, all that an IPv4 hash reads.  Toeplitz is linear in the key, so the
 * neighbour's hash is the key's own hash XOR 32 consecutive bits of the tuple -- no table per
 * neighbour: one launch hashes every tuple once per group of up to 32 neighbours and derives
 * the group's queues with a funnel shift and a XOR each.  Key bit 127 feeds no hash, so row
 * 127 holds the counts of `key` itself.
 * d_counts: RSS_KEY_NEIGHBOURS x nqueues uint64, row j = neighbour j, overwritten (cleared by
 * a kernel of the same call, then counted: the call can be captured into a graph); queue =
 * hash % htable % nqueues and columns [min(htable, nqueues), nqueues) are zero, as for
 * rss_key_search_device.  Exact for any htable, nqueues >= 1: up to 1259 queues are counted in
 * lane-private LDS bins (32 neighbours per workgroup up to 39 queues, 16 up to 78, ...), up
 * to 40288 in shared LDS bins, more by global atomics.  Any tuple alignment works; 16-byte
 * aligned tuples take the 4-tuples-per-lane path.  n == 0 only clears the counts.
 * RSS_EINVAL, before any device work, with rss_last_error naming the cause: key or counts
 * NULL; n > 0 with tuples NULL; htable or nqueues 0; key->len < 16 (a shorter key wraps in
 * its windows and a flipped bit is no longer one 32-bit delta); a key whose window[] is not
 * that of its own bytes[], i.e. one that rss_key_select_fields changed.  Field-selected keys
 * are out of scope; IPv6 tuples: rss_key_neighbourhood6_device.
 */
#define RSS_KEY_NEIGHBOURS 128
int rss_key_neighbourhood_device(const rss_key* key, const rss_tuple4* d_tuples, size_t n,
                                 uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                                 void* stream);

/*
 * Key search by load: rss_key_search_device and rss_key_neighbourhood_device with a weight per
 * tuple -- the packets or bytes of the flow -- so that a key is judged by the load it puts on
 * each queue, not by the number of flows.  d_weights: n uint32 in device memory, d_weights[i]
 * the weight of tuple i (an array of its own: resident tuple buffers are reused as they are).
 * d_loads: nkeys x nqueues (search; row k = key k) or RSS_KEY_NEIGHBOURS x nqueues
 * (neighbourhood; row j = key bit j flipped, row 127 the key itself) uint64, overwritten:
 * d_loads[k][q] is the exact sum of d_weights[i] over the tuples with hash_k(i) % htable %
 * nqueues == q.  Exact for any u32 weights (0 and 0xFFFFFFFF included), any htable, nqueues >=
 * 1, any n and any 4-byte aligned pointers: the LDS bins are 64-bit (lane-private bins for 8
 * keys per workgroup up to 77 queues, 4 up to 154, pairs up to 80, shared bins up to 2560; the
 * neighbourhood's 32 neighbours per workgroup up to 19 queues, 16 up to 39, ... 1 up to 629,
 * shared bins up to 20144), and past them every (tuple, key) is one global 64-bit atomic add.
 * Columns [min(htable, nqueues), nqueues) are zero.  With every weight 1 the loads are the
 * unweighted entry's counts.  Tuples and weights both 16-byte aligned take the 4-tuples-per-lane
 * path.  The loads are cleared by a kernel of the same call (n == 0 only clears), so both
 * entries can be captured into a graph.
 * RSS_EINVAL, before any device work, with rss_last_error naming the entry and the cause:
 * whatever the unweighted entry refuses (windows, key or loads NULL; nkeys == 0; n > 0 with
 * tuples NULL; htable or nqueues 0; for the neighbourhood key->len < 16 or a field-selected
 * key), and n > 0 with weights NULL.  IPv6 tuples are out of scope.
 */
int rss_key_search_weighted_device(const uint32_t* d_windows, size_t nkeys,
                                   const rss_tuple4* d_tuples, const uint32_t* d_weights, size_t n,
                                   uint32_t htable, uint32_t nqueues, uint64_t* d_loads,
                                   void* stream);
int rss_key_neighbourhood_weighted_device(const rss_key* key, const rss_tuple4* d_tuples,
                                          const uint32_t* d_weights, size_t n, uint32_t htable,
                                          uint32_t nqueues, uint64_t* d_loads, void* stream);

/*
 * Key search over time: the load each key puts on each queue in each time window of a packet
 * stream -- what a total per queue cannot show: two heavy flows on one queue in the same
 * second.  One row per packet: d_tuples[i], its weight d_weights[i] (n uint32, or NULL for 1
 * per packet) and its window d_slots[i] (n uint32).  d_loads: nkeys x nslots x nqueues uint64,
 * overwritten: d_loads[k][s][q] is the exact sum of the weights of the packets with slot == s
 * and hash_k % htable % nqueues == q.  A packet whose slot is >= nslots is counted nowhere;
 * columns [min(htable, nqueues), nqueues) are zero.  Exact for any u32 weights, any htable,
 * nqueues >= 1, any n, any 4-byte aligned pointers and any order of the slots.  Time order is
 * what makes it fast: a workgroup walks one contiguous tile of packets and keeps 64-bit LDS
 * bins for the slots [s, s + S) from its first packet's slot s on; a packet outside them is one
 * global 64-bit atomic per key.  With q = min(htable, nqueues) and S = the slots whose bins fit:
 *   power-of-two htable <= 65536 (158464 B of bins; lane-private rows of 256 B)
 *     8 keys per workgroup (htable <= 256)  q <= 38     (S = 3 at q = 24)
 *     4 keys                                q <= 77     (S = 6 at q = 24)
 *     2 keys                                q <= 154
 *     4 keys, shared bins of 8 B            q <= 2476
 *   any other htable (40960 B of bins, 2 keys per workgroup)
 *     lane-private rows                     q <= 40
 *     shared bins                           q <= 1280
 *   past those one global atomic per (packet, key).
 * Keys per workgroup are halved until S >= 2, and while half would still hold all nkeys.
 * Tuples, slots and (if given) weights all 16-byte aligned take the 4-packets-per-lane path.
 * The loads are cleared by a kernel of the same call (n == 0 only clears), so the entry can be
 * captured into a graph.
 * RSS_EINVAL, before any device work, with rss_last_error naming the entry and the cause:
 * windows, loads or slots NULL; nkeys == 0; nslots == 0; n > 0 with tuples NULL; htable or
 * nqueues 0.  IPv6 tuples are out of scope.
 */
int rss_key_search_timeline_device(const uint32_t* d_windows, size_t nkeys,
                                   const rss_tuple4* d_tuples, const uint32_t* d_weights,
                                   const uint32_t* d_slots, size_t n, uint32_t nslots,
                                   uint32_t htable, uint32_t nqueues, uint64_t* d_loads,
                                   void* stream);

/*
 * Key search by backlog: the deepest each queue's ring gets under each key -- what a NIC ring
 * and its core see, whatever window a timeline would be cut into.  One row per packet, in time
 * order: d_tuples[i], its weight d_weights[i] (n uint32, or NULL for 1 per packet) and its tick
 * d_ticks[i] (n uint32, non-decreasing).  Every queue drains `drain` weight units per tick
 * (0 <= drain < 2^31).  Under key k packet i joins queue q = hash_k % htable % nqueues, whose
 * backlog just after it is
 *     B = max(B_prev - drain * (d_ticks[i] - tick_prev), 0) + weight
 * (B_prev, tick_prev: the queue's previous packet; B = 0 before its first).  d_peaks: nkeys x
 * nqueues uint64, overwritten: d_peaks[k][q] is the largest B queue q reaches, 0 if it gets no
 * packet; columns [min(htable, nqueues), nqueues) are zero.  Exact in 64-bit integers for any
 * u32 weights and ticks, any htable, n < 2^31 and any 4-byte aligned pointers; packets of equal
 * ticks may come in any order; with drain == 0 the peak is the queue's load
 * (rss_key_search_weighted_device).  Ticks that decrease are a broken precondition: the peaks
 * are then unspecified, but ticks are only ever used in arithmetic, never as an index.
 * Two kernels and no waiting between workgroups: the stream is cut into at most min(ceil(n /
 * 256), 8192) segments of consecutive packets, each reduced to four 64-bit values per (key,
 * queue) by one lane stepping through the segment's staged queue ids, and a second kernel chains
 * the segments in order (rss_backlog.hip).  With q = min(htable, nqueues):
 *   power-of-two htable <= 256, nkeys > 4, q <= 128      8 keys per workgroup
 *   power-of-two htable <= 65536, nkeys > 1, q <= 255    4 keys
 *   anything else                                        1 key; its states in LDS past q = 1024
 *   q > 4096 is refused.
 * d_workspace: workspace_bytes >= rss_key_search_backlog_workspace_bytes(nkeys, n, htable,
 * nqueues) bytes of 8-byte aligned device memory, any contents, used by one call at a time; the
 * size is a function of those four arguments alone.  The call is stream-ordered, allocates
 * nothing and waits for nothing, so it can be captured into a graph; n == 0 only clears.
 * RSS_EINVAL, before any device work, with rss_last_error naming the entry and the cause:
 * windows, peaks or ticks NULL; nkeys == 0; n > 0 with tuples NULL; htable or nqueues 0; drain
 * >= 2^31; n >= 2^31; min(htable, nqueues) > 4096; a workspace that is NULL, misaligned or too
 * small (the message gives the bytes needed); for the size function a NULL out.  IPv6 tuples are
 * out of scope.
 */
int rss_key_search_backlog_workspace_bytes(size_t nkeys, size_t n, uint32_t htable,
                                           uint32_t nqueues, size_t* out);
int rss_key_search_backlog_device(const uint32_t* d_windows, size_t nkeys,
                                  const rss_tuple4* d_tuples, const uint32_t* d_weights,
                                  const uint32_t* d_ticks, size_t n, uint32_t drain,
                                  uint32_t htable, uint32_t nqueues, uint64_t* d_peaks,
                                  void* d_workspace, size_t workspace_bytes, void* stream);

/*
 * Symmetric RSS: rank the keys that hash both directions of a connection to one queue.  A key
 * with a 16-bit period (DPDK's 6d:5a:6d:5a:... is pattern 0x6d5a) has window[i] depending only
 * on i % 16, so a tuple's hash depends only on f, the XOR of its 16-bit half-words: with f_r =
 * bit 15 - r of f and p the pattern, g = XOR over r with f_r set of rotl16(p, r) and hash =
 * (g << 16) | g.  Any flow set -- IPv4 or IPv6, weighted or not -- therefore collapses into a
 * histogram of RSS_SYMMETRIC_PATTERNS fold values, and all 65536 patterns are scored from it
 * in 2^32 (fold, pattern) evaluations whatever n is.
 *
 * rss_symmetric_key: key[i] = pattern >> 8 (i even) or pattern & 0xFF (i odd) -- the literal
 * key to program; len even, RSS_KEY_MIN_BYTES..RSS_KEY_MAX_BYTES.
 * rss_symmetric_fold_device: d_tuples n tuples of `words` host-order words (3: rss_tuple4, 9:
 * rss_tuple6); `fields` a set of RSS_FIELD_* bits (1..15; every field is a multiple of 16 bits,
 * so leaving one out only masks its half-words); d_weights n uint32 or NULL (every weight 1);
 * d_folds RSS_SYMMETRIC_PATTERNS uint64: d_folds[f] = the sum of the weights of the tuples
 * that fold to f, overwritten unless flags has RSS_FLAG_ACCUMULATE (the only flag honoured), so
 * that batches -- and an IPv4 and an IPv6 capture -- can be summed.  Exact for any u32 weights
 * and any n.  Tuples and weights both 16-byte aligned take the 4-tuples-per-lane path.
 * rss_symmetric_search_device: d_loads npatterns x nqueues uint64, row r = pattern
 * first_pattern + r, overwritten: d_loads[r][q] = the sum of d_folds[f] over the f with
 * ((g(f, p) * 0x10001) % htable) % nqueues == q -- the loads under rss_symmetric_key(p).
 * Exact for any htable, nqueues >= 1: lane-private 64-bit LDS bins for 8 patterns per
 * workgroup up to 79 queues (power-of-two htable <= 256), for 4 up to 159, shared bins up to
 * 5088, global 64-bit atomics past them.  Columns [min(htable, nqueues), nqueues) are zero.
 * Both device entries are stream-ordered and clear their output by a kernel of the same call
 * (n == 0 only clears), so they can be captured into a graph.
 * rss_symmetric_search_host: the fold and the scan on host buffers under the context's lock,
 * as rss_key_search_host; synchronous; n == 0 zeroes h_loads on the host.
 * RSS_EINVAL, before any device work, with rss_last_error naming the entry and the cause: a
 * NULL folds, loads or ctx pointer; n > 0 with NULL tuples; words not 3 or 9; fields 0 or > 15;
 * npatterns == 0 or first_pattern + npatterns > 65536; htable or nqueues 0; for
 * rss_symmetric_key a NULL key or an odd or out-of-range len.
 */
#define RSS_SYMMETRIC_PATTERNS 65536u   /* also the number of fold values */
int rss_symmetric_key(uint16_t pattern, uint8_t* key, size_t len);
int rss_symmetric_fold_device(const void* d_tuples, uint32_t words, uint32_t fields,
                              const uint32_t* d_weights, size_t n, uint64_t* d_folds,
                              uint32_t flags, void* stream);
int rss_symmetric_search_device(const uint64_t* d_folds, uint32_t first_pattern,
                                uint32_t npatterns, uint32_t htable, uint32_t nqueues,
                                uint64_t* d_loads, void* stream);

/*
 * Flow aggregation: packets to the flows the weighted entries above take.  Groups n tuples
 * (d_tuples: `words` host-order words each, 3: rss_tuple4, 9: rss_tuple6) by value and sums a
 * weight per group: d_weights n uint32, or NULL for 1 per packet (the loads are then packet
 * counts).  Output, every buffer sized for n: *d_nflows (device memory) = F, the number of
 * distinct tuples; d_flows[F] the distinct tuples in first-seen order; d_loads[F] the exact
 * 64-bit sum of each flow's weights; d_first[F] the index of each flow's first packet (strictly
 * increasing).  A pure function of the input: bit-exact, whatever the scheduling.
 * A hash set of packet indices (linear probing; claim by compare-and-swap, all words compared,
 * atomic minimum: no lane ever waits for another) behind a per-workgroup LDS combiner, then a
 * count / scan / emit compaction; DESIGN.md §7. d_workspace: workspace_bytes >=
 * rss_flow_aggregate_workspace_bytes(n, words) bytes of 8-byte aligned device memory, any
 * contents (the call clears what it uses by a kernel, so it can be captured into a graph), used
 * by one call at a time.  Tuples and weights both 16-byte aligned take dwordx4 loads.  n == 0
 * only writes *d_nflows = 0 (tuples, flows, loads and first may be NULL).
 * rss_flow_aggregate_host: the same on host buffers under the context's lock (h_flows, h_loads,
 * h_first sized for n; only *nflows rows are written).  Synchronous.
 * RSS_EINVAL, before any device work, with rss_last_error naming the entry and the cause: words
 * not 3 or 9; n > 2^30; a NULL pointer other than weights (and, with n == 0, other than the
 * workspace and nflows); a workspace that is misaligned or too small; a NULL ctx.
 */
int rss_flow_aggregate_workspace_bytes(size_t n, uint32_t words, size_t* out);
int rss_flow_aggregate_device(const void* d_tuples, uint32_t words, const uint32_t* d_weights,
                              size_t n, void* d_flows, uint64_t* d_loads, uint32_t* d_first,
                              uint64_t* d_nflows, void* d_workspace, size_t workspace_bytes,
                              void* stream);

/*
 * IPv6.  36-byte input = src addr (16 B) | dst addr (16 B) |
 * src port | dst port, the layout of the Microsoft RSS IPv6 hash; stored as nine
 * host-order words whose big-endian bytes are that input (w[0..3] src, w[4..7]
 * dst, w[8] = sport << 16 | dport).  288 input bits use key bits up to 319, which
 * a 40-byte key covers without wrapping.  Fields for rss_key6_select_fields use
 * the same RSS_FIELD_* bits (RSS_FIELDS_IP = the "IPv6 only" hash).  Flags as for
 * rss_hash_device (d_queue holds uint32, or uint16 / uint8 with RSS_FLAG_QUEUE_U16 /
 * RSS_FLAG_QUEUE_U8); rss_hash6_host writes uint32 queues.
 */
#define RSS_INPUT6_BITS 288
typedef struct rss_tuple6 {
    uint32_t w[9];
} rss_tuple6;

typedef struct rss_key6 {
    uint32_t len;
    uint32_t window[RSS_INPUT6_BITS];
} rss_key6;

int rss_key6_prepare(const uint8_t* key, size_t len, rss_key6* out);
int rss_key6_select_fields(rss_key6* key, uint32_t fields);
int rss_hash6_device(const rss_key6* key, const rss_tuple6* d_tuples, size_t n,
                     uint32_t htable, uint32_t nqueues, uint32_t* d_hash, void* d_queue,
                     uint64_t* d_counts, uint32_t flags, void* stream);
/* rss_hash6_device with single-pass counts, as rss_hash_device_ws: d_workspace is a zeroed,
 * 8-byte aligned device buffer of rss_counts_workspace_bytes(nqueues) bytes used by one launch
 * at a time (every launch leaves it zero); the kernel's last workgroup writes the counts, so
 * no zeroing launch runs before it, and launches of >= 2^24 tuples hand their last rows out
 * per workgroup slot (the balanced tail) -- the IPv6 counterpart of the IPv4 bench step. */
int rss_hash6_device_ws(const rss_key6* key, const rss_tuple6* d_tuples, size_t n,
                        uint32_t htable, uint32_t nqueues, uint32_t* d_hash, void* d_queue,
                        uint64_t* d_counts, uint32_t flags, uint64_t* d_workspace, void* stream);

/*
 * Key search over IPv6 tuples: rss_key_search_device's contract for 36-byte tuples and the
 * 288 windows of an rss_key6.  d_windows: nkeys x RSS_INPUT6_BITS uint32 in device memory,
 * key k's rss_key6::window at k*288 -- a field-selected key (rss_key6_select_fields) is just
 * other windows, so it works.  d_counts: nkeys x nqueues uint64, row k = key k, overwritten
 * (cleared by a kernel of the same call); queue = hash % htable % nqueues and columns
 * [min(htable, nqueues), nqueues) are zero.  One launch per 65535 key groups: a workgroup
 * builds 63 conflict-free tables of 8-byte entries shared by its 8 keys (power-of-two htable
 * <= 256, up to 144 queues), 4 keys (power-of-two htable <= 65536, up to 288 queues) or 2 keys
 * (any htable; lane-private LDS bins up to 577 queues, shared LDS bins up to 18464, global
 * atomics beyond) and histograms its share of the tuples.  Exact for any htable, nqueues >= 1,
 * any n (0 only clears) and any 4-byte aligned tuple pointer; 16-byte aligned tuples take the
 * 4-tuples-per-lane path.  RSS_EINVAL, before any device work, with rss_last_error naming the
 * entry and the cause: windows or counts NULL; nkeys == 0; n > 0 with tuples NULL; htable or
 * nqueues 0.
 */
int rss_key_search6_device(const uint32_t* d_windows, size_t nkeys,
                           const rss_tuple6* d_tuples, size_t n, uint32_t htable,
                           uint32_t nqueues, uint64_t* d_counts, void* stream);

/*
 * A 40-byte key's single-bit-flip neighbourhood over IPv6 tuples, as
 * rss_key_neighbourhood_device: the RSS_KEY6_NEIGHBOURS keys that differ from `key` in one of
 * the 320 bits an IPv6 hash can read.  With X the 288-bit integer whose bit i is input bit i
 * and R = X << 31 (319 bits), hash(key ^ bit j, x) = hash(key, x) ^ ((R >> j) & 0xFFFFFFFF);
 * key bit 319 feeds no hash, so row 319 holds the counts of `key` itself.
 * d_counts: RSS_KEY6_NEIGHBOURS x nqueues uint64, row j = neighbour j, overwritten (cleared by
 * a kernel of the same call: capturable into a graph); columns [min(htable, nqueues), nqueues)
 * are zero.  Exact for any htable, nqueues >= 1: up to 1217 queues in lane-private LDS bins (32
 * neighbours per workgroup up to 38 queues, 16 up to 76, ...), up to 38944 in shared LDS bins,
 * more by global atomics.  Any 4-byte tuple alignment; n == 0 only clears the counts.
 * RSS_EINVAL, before any device work, with rss_last_error naming the entry and the cause: key
 * or counts NULL; n > 0 with tuples NULL; htable or nqueues 0; key->len < 40 (a shorter key
 * wraps inside its 288 windows and a flipped bit is no longer one 32-bit delta); a key whose
 * windows are not a plain Toeplitz sequence (window[i + 1] >> 1 != window[i] & 0x7FFFFFFF for
 * some i), which is how a key changed by rss_key6_select_fields shows.
 */
#define RSS_KEY6_NEIGHBOURS 320
int rss_key_neighbourhood6_device(const rss_key6* key, const rss_tuple6* d_tuples, size_t n,
                                  uint32_t htable, uint32_t nqueues, uint64_t* d_counts,
                                  void* stream);

/*
 * A key's byte neighbourhood (key search's wider local step; keysearch.refine(step="byte")
 * descends on it): the per-queue counts of the same n device-resident tuples under every key
 * that differs from `key` in one byte -- all 256 values of each of bytes [first_byte,
 * first_byte + nbytes) of the RSS_KEY_BYTES (IPv6: RSS_KEY6_BYTES) bytes a hash reads, the way
 * NICs are programmed (ethtool -X hkey aa:bb:...).  A byte's 256 values cover every change of
 * up to 8 bits inside it, its 8 single-bit flips among them.  Toeplitz is linear in the key:
 * with d = v ^ key[B], hash(key[B := v], x) = hash(key, x) ^ XOR over the set bits 0x80 >> k of
 * d of delta_{8B+k}(x), the single-bit entries' deltas; one launch hashes every tuple once per
 * chunk of up to 32 values and walks the chunk in Gray-code order, one XOR per value.
 * d_counts: nbytes * 256 x nqueues uint64, overwritten (cleared by a kernel of the same call,
 * then counted: the call can be captured into a graph): row 256 * (B - first_byte) + v holds
 * the counts under the key whose byte B is v and whose other bytes are unchanged, so row
 * 256 * (B - first_byte) + key[B] is the key itself for every B.  Key bit 127 (IPv6: 319) feeds
 * no hash: rows v and v ^ 1 of byte 15 (IPv6: 39) are equal.  queue = hash % htable % nqueues
 * and columns [min(htable, nqueues), nqueues) are zero.  The weighted entry writes d_loads, the
 * exact 64-bit sums of the u32 weights (d_weights: n uint32, any values), instead.
 * Exact for any htable, nqueues >= 1, any n (0 only clears) and any 4-byte aligned pointers;
 * tuples (and weights) 16-byte aligned take the 4-tuples-per-lane path.  Bins as the single-bit
 * entries: lane-private LDS bins for 32 values per workgroup up to 39 queues (IPv6 38, weighted
 * 19), 16 up to 78 (76, 39), ... 1 up to 1259 (1217, 629), shared LDS bins up to 40288 (38944,
 * 20144), global 64-bit atomics past them.
 * RSS_EINVAL, before any device work, with rss_last_error naming the entry and the cause:
 * whatever the matching single-bit entry refuses (key, counts or loads NULL; n > 0 with tuples
 * or weights NULL; htable or nqueues 0; key->len < 16 (IPv6: < 40); a field-selected or
 * non-plain key), and nbytes == 0 or first_byte + nbytes > 16 (IPv6: > 40).  IPv6 tuples with
 * weights are out of scope.
 */
#define RSS_KEY_BYTES 16    /* key bytes an IPv4 hash reads  */
#define RSS_KEY6_BYTES 40   /* ... an IPv6 hash reads        */
int rss_key_byte_neighbourhood_device(const rss_key* key, uint32_t first_byte, uint32_t nbytes,
                                      const rss_tuple4* d_tuples, size_t n, uint32_t htable,
                                      uint32_t nqueues, uint64_t* d_counts, void* stream);
int rss_key_byte_neighbourhood6_device(const rss_key6* key, uint32_t first_byte, uint32_t nbytes,
                                       const rss_tuple6* d_tuples, size_t n, uint32_t htable,
                                       uint32_t nqueues, uint64_t* d_counts, void* stream);
int rss_key_byte_neighbourhood_weighted_device(const rss_key* key, uint32_t first_byte,
                                               uint32_t nbytes, const rss_tuple4* d_tuples,
                                               const uint32_t* d_weights, size_t n,
                                               uint32_t htable, uint32_t nqueues,
                                               uint64_t* d_loads, void* stream);

/*
 * Host-memory convenience path (CSV in -> CSV out): owns device buffers.
 * Thread safety: any number of host threads may call the entry points that take one
 * context at once; each call holds the context's lock from entry to return, so calls on
 * one context run one after another (each with its own results) and calls on different
 * contexts run concurrently.  Replaces the reentrancy of the reference's per-call
 * Toeplitz.compute_hash (rss_simulator/toeplitz.py:59 copies the key on every call).
 * rss_ctx_destroy must not race a call on the same context.  Output that a call leaves in
 * context-owned memory (rss_csv_hash_text's file image) is valid until the next call on
 * that context, whichever thread makes it.  A call that fails returns only after every
 * copy and kernel it queued has finished: the caller's buffers are its own again.
 */
typedef struct rss_ctx rss_ctx;

int rss_ctx_create(int device, rss_ctx** out);
void rss_ctx_destroy(rss_ctx* ctx);

/*
 * Same contract as rss_hash_device but on host buffers: chunked
 * H2D -> kernel -> D2H through pinned staging, synchronous on return.
 * h_hash / h_queue (uint32) / h_counts may be NULL; only RSS_FLAG_ACCUMULATE
 * is honoured.  Buffers that are already page-locked (rss_host_alloc,
 * hipHostMalloc, hipHostRegister) are copied by DMA directly, without the
 * staging copy; pageable buffers go through the context's pinned staging.
 */
int rss_hash_host(rss_ctx* ctx, const rss_key* key, const rss_tuple4* h_tuples,
                  size_t n, uint32_t htable, uint32_t nqueues, uint32_t* h_hash,
                  uint32_t* h_queue, uint64_t* h_counts, uint32_t flags);

/*
 * Page-locked host memory for rss_hash_host's direct-DMA path (hipHostMalloc).
 * Pinning costs far more than a copy, so allocate once and reuse across batches.
 * rss_host_free(NULL) is a no-op.
 */
int rss_host_alloc(size_t bytes, void** out);
void rss_host_free(void* p);

/*
 * ---- CSV fast path (host, multi-threaded) ----
 * Replaces pd.read_csv (rss_simulator/simulator.py:55) and the two to_csv calls
 * of write_statistics (simulator.py:114-115) for CANONICAL files: header = the
 * four columns src_ip,dst_ip,src_port,dst_port in any order and nothing else;
 * rows = four unquoted fields, dotted-quad addresses with octets 0..255 and no
 * leading zeros, ports 0..65535 in plain decimal; LF or CRLF; empty lines
 * skipped; ASCII only.  pandas round-trips such fields unchanged, so the output
 * is byte-identical to the reference's.  Any other file -> RSS_ENOTSUP: the
 * caller must take the pandas path, which reproduces the reference's parsing
 * and error behaviour.  `threads` <= 0 picks min(16, hardware threads).
 */
typedef struct rss_csv_layout {
    uint8_t field_column[4]; /* field f of a row holds column field_column[f]:
                                0 src_ip, 1 dst_ip, 2 src_port, 3 dst_port   */
} rss_csv_layout;

/* Parse the whole file image; RSS_EINVAL with *n_rows set if cap is too small. */
int rss_csv_parse(const char* data, size_t len, rss_tuple4* tuples, size_t cap,
                  size_t* n_rows, rss_csv_layout* layout, int threads);

/* Upper bound of rss_csv_format's output size. */
size_t rss_csv_format_bound(size_t n, uint32_t nqueues);

/*
 * An address column of a DataFrame (Simulator.calc_hash on pandas data, whatever file or
 * frame it came from): `text` holds its n cells joined by '\n'.  Cell i that is a plain
 * quad -- four dot-separated runs of 1-3 ASCII digits, nothing else -- gets ok[i] = 1 (2 when
 * it is also canonical: octets 0..255 without leading zeros, the text rss_csv_format writes
 * back, so a write_statistics of such cells may take the native formatter) and
 * out[i] = (o0 << 24 | o1 << 16 | o2 << 8 | o3) mod 2^32 with the octets NOT range-checked
 * and OR-combined, exactly __ip_to_int + the byte masks of __prepare_input_bytes
 * (rss_simulator/toeplitz.py:100-111, :127-137); any other cell gets ok[i] = 0 and the caller
 * converts it with the reference's own rules (whitespace, extra octets, errors).  RSS_EINVAL
 * when the text does not hold exactly n cells (a cell containing '\n').
 */
int rss_parse_dotted(const char* text, size_t len, size_t n, uint32_t* out, uint8_t* ok);

/*
 * The same for an IPv6 address column (the additive --ipv6 input): cell i that is RFC 4291
 * text without an embedded IPv4 part or zone (1-4 hex digits per group, at most one '::';
 * the CSV path's canonical IPv6 form) gets ok[i] = 1 and out[4i..4i+3] = its 128 bits as four
 * big-endian-valued words, as ipaddress.IPv6Address reads it; any other cell ok[i] = 0.
 */
int rss_parse_ipv6(const char* text, size_t len, size_t n, uint32_t* out, uint8_t* ok);

/*
 * Write the statistics file of write_statistics (simulator.py:100-115): the
 * "queue_number,counts" rows of the non-empty queues, then the table with the
 * input columns in input order plus hash_result,queue_number.  `cap` must be
 * >= rss_csv_format_bound(n, nqueues).
 */
int rss_csv_format(const rss_tuple4* tuples, const uint32_t* hash, const uint32_t* queue,
                   size_t n, const uint64_t* counts, uint32_t nqueues,
                   const rss_csv_layout* layout, char* out, size_t cap, size_t* out_len,
                   int threads);

/*
 * IPv6 rows through the same fast path (the --ipv6 input of SURVEY.md §8f row 4;
 * pandas path: Simulator with ipv6, ingest.pack_frame6).  Canonical IPv6 fields are
 * RFC 4291 text without an embedded IPv4 part or zone id (1-4 hex digits per group,
 * at most one "::"); ports and the header as above.  rss_csv_parse6 fills tuples[n]
 * and spans[2n] (byte offsets of each row's text, line end excluded); pandas keeps
 * the address strings verbatim, so rss_csv_format6 writes each row as its input text
 * + ",hash,queue" after the same counts prefix.  Same return codes as the IPv4 pair.
 */
int rss_csv_parse6(const char* data, size_t len, rss_tuple6* tuples, uint64_t* spans, size_t cap,
                   size_t* n_rows, rss_csv_layout* layout, int threads);
size_t rss_csv_format6_bound(const uint64_t* spans, size_t n, uint32_t nqueues);
int rss_csv_format6(const char* data, const uint64_t* spans, const uint32_t* hash,
                    const uint32_t* queue, size_t n, const uint64_t* counts, uint32_t nqueues,
                    const rss_csv_layout* layout, char* out, size_t cap, size_t* out_len,
                    int threads);

/*
 * ---- CSV on the device ----
 * The whole `--csv` job for a CANONICAL file image (the rules above): the body goes
 * to the device once, newlines are indexed, rows parsed, hashed (rss_hash_device or,
 * with `reta`, rss_hash_device_reta), and the statistics file of write_statistics is
 * formatted there; the header and per-queue count lines are built on the host.
 * Replaces pd.read_csv (simulator.py:55), calc_hash / calc_queue_number (:74-98)
 * and write_statistics (:100-115).  On success *out / *out_len is the file image
 * in ctx-owned host memory, valid until the next call on ctx; counts (nqueues
 * uint64) and *n_rows are set.  RSS_CSV_COUNTS_ONLY skips the per-row outputs
 * and the file (out / out_len may be NULL).  Non-canonical input or a body of 4 GiB
 * or more -> RSS_ENOTSUP (take the host or pandas path).
 */
#define RSS_CSV_COUNTS_ONLY 1u
int rss_csv_hash_text(rss_ctx* ctx, const rss_key* key, const char* text, size_t len,
                      uint32_t htable, uint32_t nqueues, const uint32_t* reta, uint32_t flags,
                      const char** out, size_t* out_len, uint64_t* counts, size_t* n_rows);

/*
 * rss_csv_hash_text from file to file: the input streams through two pinned staging
 * buffers of ctx (read of chunk k+1 overlaps the upload of chunk k) and the output
 * rows stream back the same way (download of chunk k+1 overlaps the write of chunk
 * k), so no file-sized host buffer exists.  Bodies of any size are processed in
 * line-aligned segments below 4 GiB (3 GiB; RSS_CSV_SEGMENT_BYTES lowers it), counts
 * summed over the segments and rows written after the last one.  out_path may be NULL with
 * RSS_CSV_COUNTS_ONLY.  An unreadable input or an output that cannot be created is
 * RSS_ENOTSUP as well: the pandas path then raises the reference's error.
 */
int rss_csv_hash_file(rss_ctx* ctx, const rss_key* key, const char* in_path, const char* out_path,
                      uint32_t htable, uint32_t nqueues, const uint32_t* reta, uint32_t flags,
                      uint64_t* counts, size_t* n_rows);

/*
 * The IPv6 `--ipv6 --csv` job on the device, same contracts as rss_csv_hash_text /
 * rss_csv_hash_file: rows are the canonical IPv6 form of rss_csv_parse6 (RFC 4291 text,
 * no embedded IPv4 or zone), hashed with rss_hash6_device (or rss_hash6_device_reta),
 * and each output row is the input row's own text plus ",hash,queue" -- the bytes
 * rss_csv_format6 writes, which are the pandas path's (ingest.py / simulator.py:100-115).
 */
int rss_csv6_hash_text(rss_ctx* ctx, const rss_key6* key, const char* text, size_t len,
                       uint32_t htable, uint32_t nqueues, const uint32_t* reta, uint32_t flags,
                       const char** out, size_t* out_len, uint64_t* counts, size_t* n_rows);
int rss_csv6_hash_file(rss_ctx* ctx, const rss_key6* key, const char* in_path,
                       const char* out_path, uint32_t htable, uint32_t nqueues,
                       const uint32_t* reta, uint32_t flags, uint64_t* counts, size_t* n_rows);

/* rss_key_search_device on host buffers (keys: nkeys prepared keys; h_counts:
 * nkeys x nqueues uint64).  Synchronous. */
int rss_key_search_host(rss_ctx* ctx, const rss_key* keys, size_t nkeys,
                        const rss_tuple4* h_tuples, size_t n, uint32_t htable,
                        uint32_t nqueues, uint64_t* h_counts);

/* rss_key_neighbourhood_device on host buffers (h_counts: RSS_KEY_NEIGHBOURS x nqueues
 * uint64), as rss_key_search_host: takes the context's lock, uploads the tuples, launches,
 * copies the counts back.  Synchronous.  The same validation (and a NULL ctx) is refused
 * first; n == 0 zeroes h_counts on the host. */
int rss_key_neighbourhood_host(rss_ctx* ctx, const rss_key* key, const rss_tuple4* h_tuples,
                               size_t n, uint32_t htable, uint32_t nqueues, uint64_t* h_counts);

/* rss_key_search_weighted_device / rss_key_neighbourhood_weighted_device on host buffers
 * (keys: nkeys prepared keys; h_weights: n uint32; h_loads: nkeys x nqueues /
 * RSS_KEY_NEIGHBOURS x nqueues uint64), as rss_key_search_host: takes the context's lock,
 * uploads the tuples and the weights, launches, copies the loads back.  Synchronous.  The same
 * validation (and a NULL ctx, or a key that was not prepared) is refused first; n == 0 zeroes
 * h_loads on the host. */
int rss_key_search_weighted_host(rss_ctx* ctx, const rss_key* keys, size_t nkeys,
                                 const rss_tuple4* h_tuples, const uint32_t* h_weights, size_t n,
                                 uint32_t htable, uint32_t nqueues, uint64_t* h_loads);
int rss_key_neighbourhood_weighted_host(rss_ctx* ctx, const rss_key* key,
                                        const rss_tuple4* h_tuples, const uint32_t* h_weights,
                                        size_t n, uint32_t htable, uint32_t nqueues,
                                        uint64_t* h_loads);

/* rss_key_search_timeline_device on host buffers (keys: nkeys prepared keys; h_weights: n
 * uint32 or NULL; h_slots: n uint32; h_loads: nkeys x nslots x nqueues uint64), as
 * rss_key_search_weighted_host: takes the context's lock, uploads, launches, copies the loads
 * back.  Synchronous.  The same validation (and a NULL ctx, or a key that was not prepared) is
 * refused first; n == 0 zeroes h_loads on the host. */
int rss_key_search_timeline_host(rss_ctx* ctx, const rss_key* keys, size_t nkeys,
                                 const rss_tuple4* h_tuples, const uint32_t* h_weights,
                                 const uint32_t* h_slots, size_t n, uint32_t nslots,
                                 uint32_t htable, uint32_t nqueues, uint64_t* h_loads);

/* rss_key_search_backlog_device on host buffers (keys: nkeys prepared keys; h_weights: n uint32
 * or NULL; h_ticks: n uint32, non-decreasing; h_peaks: nkeys x nqueues uint64), as
 * rss_key_search_timeline_host: takes the context's lock, uploads, launches on a workspace of
 * its own, copies the peaks back.  Synchronous.  The same validation (and a NULL ctx, or a key
 * that was not prepared) is refused first; n == 0 zeroes h_peaks on the host. */
int rss_key_search_backlog_host(rss_ctx* ctx, const rss_key* keys, size_t nkeys,
                                const rss_tuple4* h_tuples, const uint32_t* h_weights,
                                const uint32_t* h_ticks, size_t n, uint32_t drain, uint32_t htable,
                                uint32_t nqueues, uint64_t* h_peaks);

/* rss_symmetric_fold_device + rss_symmetric_search_device on host buffers (described with
 * them): h_tuples n x `words` uint32, h_weights n uint32 or NULL, h_loads npatterns x nqueues
 * uint64.  Synchronous. */
int rss_symmetric_search_host(rss_ctx* ctx, const void* h_tuples, uint32_t words, uint32_t fields,
                              const uint32_t* h_weights, size_t n, uint32_t first_pattern,
                              uint32_t npatterns, uint32_t htable, uint32_t nqueues,
                              uint64_t* h_loads);

/* rss_flow_aggregate_device on host buffers (described with it): uploads the tuples and the
 * weights, aggregates, downloads the *nflows rows.  Synchronous. */
int rss_flow_aggregate_host(rss_ctx* ctx, const void* h_tuples, uint32_t words,
                            const uint32_t* h_weights, size_t n, void* h_flows, uint64_t* h_loads,
                            uint32_t* h_first, size_t* nflows);

/* rss_key_search6_device on host buffers (keys: nkeys prepared rss_key6; h_counts: nkeys x
 * nqueues uint64), as rss_key_search_host.  Synchronous.  Refuses what the device entry
 * refuses (and a NULL ctx or keys, or a key that was not prepared) before any device work. */
int rss_key_search6_host(rss_ctx* ctx, const rss_key6* keys, size_t nkeys,
                         const rss_tuple6* h_tuples, size_t n, uint32_t htable,
                         uint32_t nqueues, uint64_t* h_counts);

/* rss_key_neighbourhood6_device on host buffers (h_counts: RSS_KEY6_NEIGHBOURS x nqueues
 * uint64), as rss_key_neighbourhood_host: the same validation (and a NULL ctx) is refused
 * first; n == 0 zeroes h_counts on the host. */
int rss_key_neighbourhood6_host(rss_ctx* ctx, const rss_key6* key, const rss_tuple6* h_tuples,
                                size_t n, uint32_t htable, uint32_t nqueues, uint64_t* h_counts);

/* The rss_key_byte_neighbourhood*_device entries on host buffers (h_counts / h_loads: nbytes *
 * 256 x nqueues uint64; h_weights: n uint32), as rss_key_neighbourhood_host: take the context's
 * lock, upload the tuples (and weights), launch, copy the rows back.  Synchronous.  The same
 * validation (and a NULL ctx) is refused first; n == 0 zeroes the output on the host. */
int rss_key_byte_neighbourhood_host(rss_ctx* ctx, const rss_key* key, uint32_t first_byte,
                                    uint32_t nbytes, const rss_tuple4* h_tuples, size_t n,
                                    uint32_t htable, uint32_t nqueues, uint64_t* h_counts);
int rss_key_byte_neighbourhood6_host(rss_ctx* ctx, const rss_key6* key, uint32_t first_byte,
                                     uint32_t nbytes, const rss_tuple6* h_tuples, size_t n,
                                     uint32_t htable, uint32_t nqueues, uint64_t* h_counts);
int rss_key_byte_neighbourhood_weighted_host(rss_ctx* ctx, const rss_key* key,
                                             uint32_t first_byte, uint32_t nbytes,
                                             const rss_tuple4* h_tuples,
                                             const uint32_t* h_weights, size_t n, uint32_t htable,
                                             uint32_t nqueues, uint64_t* h_loads);

/* rss_hash6_device on host buffers: rss_hash_host's contract and path (the same staging,
 * small-batch path, pipeline and direct DMA of page-locked buffers), 36-byte tuples. */
int rss_hash6_host(rss_ctx* ctx, const rss_key6* key, const rss_tuple6* h_tuples, size_t n,
                   uint32_t htable, uint32_t nqueues, uint32_t* h_hash, uint32_t* h_queue,
                   uint64_t* h_counts, uint32_t flags);

/*
 * ---- pcap input (host) ----
 * One packed 4-tuple per IPv4 packet of a classic libpcap image (either byte
 * order, us/ns timestamps) or a pcapng image (sections of either byte order,
 * per-interface link types, enhanced / simple / obsolete packet blocks; other
 * blocks skipped).  Link types: Ethernet incl. 802.1Q/802.1ad tags, Linux cooked
 * v1, raw IPv4.  TCP/UDP/SCTP packets carry their ports; other protocols and every
 * fragment carry ports 0 (the 2-tuple hash, as NICs do).  protocols (nullable)
 * gets the IP protocol byte per tuple.  Non-IPv4 / malformed packets, and packets
 * of interfaces with other link types, are skipped and counted in *skipped.
 * Returns RSS_ENOTSUP for other images; RSS_EINVAL with *n_out = the needed size
 * when cap is too small.
 */
int rss_pcap_parse(const uint8_t* data, size_t len, rss_tuple4* tuples, uint8_t* protocols,
                   size_t cap, size_t* n_out, size_t* skipped);

/*
 * The same captures, one rss_tuple6 per IPv6 packet (link types as above plus raw
 * IPv6): the fixed header's addresses; the extension-header chain (hop-by-hop,
 * routing, destination options, AH, fragment) is walked to the upper layer, whose
 * ports count for TCP/UDP/SCTP; fragments, ESP and other upper layers carry ports 0.
 * protocols gets the upper-layer protocol.  IPv4 and malformed packets are skipped.
 */
int rss_pcap_parse6(const uint8_t* data, size_t len, rss_tuple6* tuples, uint8_t* protocols,
                    size_t cap, size_t* n_out, size_t* skipped);

int rss_hash_host_reta(rss_ctx* ctx, const rss_key* key, const rss_tuple4* h_tuples, size_t n,
                       uint32_t htable, const uint32_t* reta, uint32_t nqueues, uint32_t* h_hash,
                       uint32_t* h_queue, uint64_t* h_counts, uint32_t flags);

/* The IPv6 counterparts: rss_hash6_device / rss_hash6_host with the bucket -> queue
 * step through reta[htable] (same limits as rss_hash_device_reta). */
int rss_hash6_device_reta(const rss_key6* key, const rss_tuple6* d_tuples, size_t n,
                          uint32_t htable, const uint32_t* reta, uint32_t nqueues,
                          uint32_t* d_hash, void* d_queue, uint64_t* d_counts, uint32_t flags,
                          void* stream);
int rss_hash6_host_reta(rss_ctx* ctx, const rss_key6* key, const rss_tuple6* h_tuples, size_t n,
                        uint32_t htable, const uint32_t* reta, uint32_t nqueues, uint32_t* h_hash,
                        uint32_t* h_queue, uint64_t* h_counts, uint32_t flags);

/*
 * Multi-GPU host batch (replaces the same rows of Simulator.calc_hash /
 * calc_queue_number / write_statistics as rss_hash_host, simulator.py:74-113).  The n
 * tuples are split into nctx contiguous ranges as sharding.shard_range splits a batch over
 * ranks (n / nctx each, the first n % nctx ranges one tuple longer);
 * context i hashes range i on its own device from its own host thread and copies the
 * hash / queue slice straight into the caller's output range (no collective), and the
 * per-queue counts of all ranges are summed on the host -- exact integers, so identical
 * to one device.  Contexts must be distinct (several may share a device).  reta is
 * NULL for the reference's `% nqueues` mapping, else htable queue ids (as
 * rss_hash_host_reta).  Only RSS_FLAG_ACCUMULATE is honoured.  Synchronous.
 */
int rss_hash_host_multi(rss_ctx* const* ctxs, int nctx, const rss_key* key,
                        const rss_tuple4* h_tuples, size_t n, uint32_t htable,
                        const uint32_t* reta, uint32_t nqueues, uint32_t* h_hash,
                        uint32_t* h_queue, uint64_t* h_counts, uint32_t flags);

/* Number of visible gfx950 devices (0 when there is no GPU). */
int rss_device_count(int* out);

/* Thread-local message describing the last failure on this thread ("" if none). */
const char* rss_last_error(void);

/* RSS_ABI_VERSION of the loaded library. */
int rss_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* RSS_TOEPLITZ_H */
