"""The flow table's hash (csrc/rss_flow_hash.h) in numpy, and its inverse in the last word: tuples
with chosen hashes, so a test can put flows on chosen slots of the aggregation's two tables.
tests/test_flow_aggregate.py holds this port to the header."""
import numpy as np

M32 = 0xFFFFFFFF
SEED = 0x2545F491
MIX_MUL, MIX_INV = 0x9E3779B1, 0x0E8B2F51  # inverses modulo 2^32
FIN1_MUL, FIN1_INV = 0x85EBCA6B, 0xA5CB9243
FIN2_MUL, FIN2_INV = 0xC2B2AE35, 0x7ED1B41D
CHUNK = {3: 3072, 9: 2048}  # AggChunk<words>::kChunk; the local table has twice as many slots
MIN_CAP = 1024  # kAggMinCap


def _mix(h, w):
    h = ((h ^ w) * MIX_MUL) & M32
    return ((h << 15) | (h >> 17)) & M32


def _state(rows):
    """The hash state (uint64 holding 32 bits) after mixing in every column of `rows`."""
    rows = np.asarray(rows, dtype=np.uint64)
    h = np.full(len(rows), SEED, dtype=np.uint64)
    for k in range(rows.shape[1]):
        h = _mix(h, rows[:, k])
    return h


def agg_hash(tuples):
    """agg_hash<words> of every row of (n, words) uint32 `tuples`, as uint32[n]."""
    h = _state(tuples)
    h ^= h >> 16
    h = (h * FIN1_MUL) & M32
    h ^= h >> 13
    h = (h * FIN2_MUL) & M32
    return (h ^ (h >> 16)).astype(np.uint32)


def preimage(prefix_words, target_hashes):
    """(n, words) uint32 tuples: the (n, words - 1) `prefix_words` and the one last word that
    gives row i the hash `target_hashes[i]` (one target for all rows if scalar)."""
    prefix = np.asarray(prefix_words, dtype=np.uint32)
    h = np.broadcast_to(np.asarray(target_hashes, dtype=np.uint64), (len(prefix),)).copy()
    h ^= h >> 16  # the finaliser, backwards
    h = (h * FIN2_INV) & M32
    h ^= (h >> 13) ^ (h >> 26)
    h = (h * FIN1_INV) & M32
    h ^= h >> 16
    h = ((h >> 15) | (h << 17)) & M32  # the last mix: rotate back, divide, xor the state out
    last = ((h * MIX_INV) & M32) ^ _state(prefix)
    return np.concatenate([prefix, last.astype(np.uint32)[:, None]], axis=1)


def capacity(n):
    """Slots of the global table for n packets: the power of two >= 2n, at least MIN_CAP."""
    cap = MIN_CAP
    while cap < 2 * n:
        cap <<= 1
    return cap


def local_slot(hashes, words):
    """Where a hash starts in the combiner's local table: umulhi(hash, 2 * kChunk)."""
    return (np.asarray(hashes, dtype=np.uint64) * (2 * CHUNK[words])) >> 32


def hash_for_slots(local, global_, words, cap):
    """One hash that starts at slot `local` of the local table and `global_` of a global table of
    `cap` slots: the top bits pick the first, the low bits the second."""
    nslots = 2 * CHUNK[words]
    lowest = -((-local << 32) // nslots)  # the first hash of the local slot
    h = -(-lowest // cap) * cap + global_
    assert h <= M32 and (h * nslots) >> 32 == local and h & (cap - 1) == global_, (local, global_, cap)
    return h
