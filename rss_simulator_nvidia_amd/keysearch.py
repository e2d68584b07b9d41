"""Key search: find RSS keys that spread a flow set evenly.

The reference can only draw one random key (``HashKey.random_hash_key``,
``rss_simulator/hash_key.py:53-60``) and show its histogram.  Here thousands of
candidate keys of the same shape (40 distinct random bytes) are evaluated in one
GPU launch (``rss_key_search_device``: one LDS lookup table per key, the flows read
from the on-die cache) and ranked by how close each key's per-queue counts come to
the ideal spread of the hash table: queue q owns ``slots(q) = #{b < H : b % Q == q}``
of the H buckets, so a perfect key gives it ``n * slots(q) / H`` flows.

    python -m rss_simulator_nvidia_amd.keysearch --ips-file flows.csv \\
        --htable-size 128 --num-queues 24 --keys 4096 --top 5 --out best_key.txt

``--refine STEPS`` then improves the best candidate (and a ``--key-file`` key) by local
search: Toeplitz is linear in the key, so all 128 single-bit flips of a key are scored in
one launch from the key's own hashes (``rss_key_neighbourhood_device``), and :func:`refine`
flips the best bit until none improves the spread.  ``--refine-step byte`` descends over whole
bytes instead: every value of every key byte in one launch (``rss_key_byte_neighbourhood_device``;
a byte's 256 values contain its 8 single-bit flips), as NIC keys are programmed.

``--ipv6`` does the same for a CSV of IPv6 flows (``rss_key_search6_device``,
``rss_key_neighbourhood6_device``: 36-byte tuples, the 320 key bits an IPv6 hash reads).

``--weight-column NAME`` (a CSV column of packets or bytes per flow) or ``--pcap PATH`` (a
capture: its unique flows, weighted by their packets) rank and refine by the **load** each
key puts on a queue instead of the number of flows (``rss_key_search_weighted_device``,
``rss_key_neighbourhood_weighted_device``; IPv4 flows).

``--aggregate`` takes a CSV with one row per **packet**: the rows are folded to flows on the
GPU (``rss_flow_aggregate_device``: a hash set of packet indices, first-seen order) and each
flow's load is the sum of its rows' ``--weight-column``, or its row count without one.
``--pcap`` de-duplicates its packets the same way.

``--time-column NAME --window WIDTH`` take a CSV with one row per packet and a numeric time:
the ranking is unchanged (rows are packets, so it is by packet load, or by ``--weight-column``),
and each listed key then gets a line ``peak P at window S of W`` -- its hottest queue in any
window, relative to the busiest window's ideal share (:func:`timeline`, :func:`peak`; one
``rss_key_search_timeline_device`` launch; IPv4).  A key that is level over the whole capture
can still put two heavy flows on one queue in the same window; the peak shows it.

``--drain UNITS --tick WIDTH`` (with ``--time-column``) add what a NIC ring sees, whatever the
window: every queue drains ``UNITS`` of load per tick of ``WIDTH`` time units, a packet arriving
at a queue raises its backlog by its weight, and each listed key gets a line ``backlog B at queue
Q`` -- the deepest any queue's backlog gets over the capture (:func:`backlog`; one
``rss_key_search_backlog_device`` call, exact in 64-bit integers; IPv4).  A burst across a
window edge or a microburst inside a wide window shows here as it is.

``--symmetric`` ranks the 65536 symmetric keys instead -- a 16-bit pattern repeated over the
key (DPDK's ``6d:5a:6d:5a:...``), which sends both directions of a connection to one queue.
Their hash depends only on the XOR of a tuple's 16-bit half-words, so the flows are folded
into a 65536-bin histogram once (``rss_symmetric_fold_device``) and every pattern is scored
from it (``rss_symmetric_search_device``): exhaustive and exact, for IPv4 or IPv6 flows,
weighted or not.
"""
import argparse
import random

import numpy as np
import pandas as pd

from rss_simulator_nvidia_amd import _native
from rss_simulator_nvidia_amd.arg_parse_types import PositiveInt
from rss_simulator_nvidia_amd.arg_parse_types import arg_parse_type_decorator as apt_decorator
from rss_simulator_nvidia_amd.hash_key import HASH_KEY_BYTES_LENGTH, HashKey
from rss_simulator_nvidia_amd.ingest import pack_frame, pack_frame6


def random_keys(count, seed=0, length=HASH_KEY_BYTES_LENGTH):
    """``count`` keys shaped like ``random_hash_key()``: ``length`` distinct random bytes."""
    rng = random.Random(seed)
    return [rng.sample(range(256), length) for _ in range(count)]


def key_text(key):
    """Colon-separated hex, the ``--key-file`` format (``hash_key.py:25-28``)."""
    return ":".join("{:02x}".format(b) for b in key)


def slot_share(htable, nqueues, width=None):
    """Fraction of the H buckets each queue owns (bucket b -> queue b % Q), for queues
    ``[0, width)`` (default: all Q)."""
    q = np.arange(nqueues if width is None else min(width, nqueues), dtype=np.int64)
    slots = htable // nqueues + (q < htable % nqueues)
    if nqueues > htable:
        slots = (q < htable).astype(np.int64)
    return slots / float(htable)


def balance(counts, htable, nqueues):
    """Per-key balance metrics for ``counts`` (``[keys, Q]``).

    Returns a dict of arrays: ``max_load`` = max over reachable queues of
    observed / ideal flows (1.0 is perfect), ``chi2`` = sum of (observed - ideal)^2 /
    ideal, and ``used`` = number of non-empty queues.

    Every row is normalised by its own sum, so rows of weighted loads (``weights=`` in
    :func:`evaluate`, :func:`neighbourhood`, ...) are ranked unchanged: "flows" then reads
    packets or bytes, whatever the weights count.
    """
    counts = np.atleast_2d(np.asarray(counts, dtype=np.float64))
    n = counts.sum(axis=1, keepdims=True)
    # Count rows are min(H, Q) wide (``_native.queue_modulus``): queues >= H own no bucket,
    # so the ideal share is cut to the columns present (nothing is lost).
    ideal = n * slot_share(htable, nqueues, counts.shape[1])[None, :]
    live = ideal[0] > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(ideal > 0, counts / np.where(ideal > 0, ideal, 1), 0.0)
        chi2 = (((counts - ideal) ** 2) / np.where(ideal > 0, ideal, 1))[:, live].sum(axis=1)
    return {"max_load": rel[:, live].max(axis=1) if live.any() else np.zeros(len(counts)),
            "chi2": chi2, "used": (counts > 0).sum(axis=1)}


def _no_ipv6_weights(ipv6, weights):
    if ipv6 and weights is not None:
        raise NotImplementedError("weights with ipv6=True: the weighted key-search kernels "
                                  "serve IPv4 tuples only")


def evaluate(keys, tuples, htable, nqueues, ctx=None, ipv6=False, weights=None):
    """uint64 per-queue counts ``[len(keys), Q]`` of packed ``tuples`` under every key (GPU);
    ``ipv6``: ``tuples`` are ``TUPLE6_DTYPE`` or ``(n, 9)`` uint32.  ``weights`` (one integer
    in [0, 2^32) per tuple, IPv4 only): per-queue loads, the sums of the weights, instead."""
    _no_ipv6_weights(ipv6, weights)
    ctx = ctx or _native.default_context()
    if ipv6:
        return ctx.key_search6([_native.prepare_key6(k) for k in keys], tuples, htable, nqueues)
    prepared = [_native.prepare_key(k) for k in keys]
    if weights is None:
        return ctx.key_search(prepared, tuples, htable, nqueues)
    return ctx.key_search(prepared, tuples, htable, nqueues, weights=weights)


def timeline(keys, tuples, slots, htable, nqueues, nslots=None, weights=None, ctx=None,
             ipv6=False):
    """uint64 loads ``[len(keys), nslots, min(H, Q)]`` of the packets ``tuples`` under every
    key, per time window (GPU, one launch: ``rss_key_search_timeline_device``): packet i falls
    into window ``slots[i]`` (an integer in [0, 2^32)) and adds ``weights[i]`` (one integer in
    [0, 2^32) per packet; 1 without ``weights``) to its queue there.  ``nslots`` defaults to
    ``slots.max() + 1``; packets in windows ``>= nslots`` are left out.  Any order of the slots
    is exact; time order is what makes it fast.  IPv4 only, like the weighted entries."""
    if ipv6:
        raise NotImplementedError("timeline with ipv6=True: the weighted key-search kernels "
                                  "serve IPv4 tuples only")
    s = _native.tuple_slots(slots, len(tuples))
    if nslots is None:
        nslots = int(s.max()) + 1 if len(s) else 1
    if int(nslots) < 1 or int(nslots) > 0xFFFFFFFF:
        raise ValueError("nslots must lie in [1, 2^32), got %r" % (nslots,))
    ctx = ctx or _native.default_context()
    return ctx.key_search_timeline([_native.prepare_key(k) for k in keys], tuples, s, int(nslots),
                                   htable, nqueues, weights=weights)


def backlog(keys, tuples, ticks, drain, htable, nqueues, weights=None, ctx=None):
    """uint64 peak backlogs ``[len(keys), min(H, Q)]`` of the time-ordered packets ``tuples``
    under every key (GPU: ``rss_key_search_backlog_device``).  Packet i arrives at tick
    ``ticks[i]`` (integers in [0, 2^32), non-decreasing) with ``weights[i]`` units (one integer
    in [0, 2^32) per packet; 1 without ``weights``); every queue drains ``drain`` units (an
    integer in [0, 2^31)) per tick; a queue's backlog after an arrival is ``max(previous -
    drain * ticks since, 0) + weight`` and the result is the largest it reaches (0 for a queue
    without packets).  ``drain=0`` gives the loads of :func:`evaluate`.  IPv4 tuples."""
    t = _native.tuple_ticks(ticks, len(tuples))
    drain = _native.backlog_drain(drain)
    ctx = ctx or _native.default_context()
    return ctx.key_search_backlog([_native.prepare_key(k) for k in keys], tuples, t, drain,
                                  htable, nqueues, weights=weights)


def peak(loads, htable, nqueues):
    """How far the hottest (window, queue) of ``loads`` (``[keys, windows, min(H, Q)]`` from
    :func:`timeline`, or one key's ``[windows, min(H, Q)]``) stands above the busiest window's
    ideal share: ``peak`` = max over (s, q) of ``loads[s, q] / slot_share[q]``, divided by the
    max over s of ``loads[s].sum()`` -- 1.0 means the busiest window was perfectly level and no
    other window's queue exceeded it; 0.0 for no load at all.  Returns a dict of per-key arrays:
    ``peak`` and ``window``, the window where it occurs."""
    loads = np.asarray(loads, dtype=np.float64)
    if loads.ndim == 2:
        loads = loads[None]
    rel = loads / slot_share(htable, nqueues, loads.shape[2])[None, None, :]
    busiest = loads.sum(axis=2).max(axis=1)
    hot = rel.max(axis=2)  # [keys, windows]
    return {"peak": np.where(busiest > 0, hot.max(axis=1) / np.where(busiest > 0, busiest, 1), 0.0),
            "window": hot.argmax(axis=1)}


def window_slots(times, width):
    """``(slots, nslots)`` of per-packet ``times``: ``slots[i] = floor((times[i] - t_min) /
    width)`` as uint32, ``width`` in the units of ``times``.  ``ValueError`` unless the times are
    finite numbers, ``width > 0`` and the windows number fewer than 2^32."""
    t = np.asarray(times)
    if t.ndim != 1 or t.dtype.kind not in "iuf":
        raise ValueError("times must be one number per packet, not %s" % t.dtype)
    if not width > 0:
        raise ValueError("the window width must be > 0, got %r" % (width,))
    t = t.astype(np.float64)
    if not np.isfinite(t).all():
        raise ValueError("times must be finite numbers")
    if len(t) == 0:
        return np.zeros(0, dtype=np.uint32), 1
    slots = np.floor((t - t.min()) / float(width))
    if slots.max() >= 2.0**32:
        raise ValueError("%g windows of width %r: more than 2^32" % (slots.max() + 1, width))
    return slots.astype(np.uint32), int(slots.max()) + 1


def search(tuples, htable, nqueues, n_keys=1024, seed=0, top=10, extra_keys=(), ipv6=False,
           weights=None):
    """Rank ``n_keys`` random candidates (plus ``extra_keys``) for ``tuples``, by flows or with
    ``weights`` by load.

    Returns a list of dicts (best first): ``key``, ``max_load``, ``chi2``, ``used``, ``counts``.
    """
    keys = [list(k) for k in extra_keys] + random_keys(n_keys, seed)
    counts = evaluate(keys, tuples, htable, nqueues, ipv6=ipv6, weights=weights)
    m = balance(counts, htable, nqueues)
    order = np.lexsort((m["chi2"], m["max_load"]))
    return [{"key": keys[i], "max_load": float(m["max_load"][i]), "chi2": float(m["chi2"][i]),
             "used": int(m["used"][i]), "counts": counts[i]} for i in order[:top]]


def symmetric_key(pattern, length=HASH_KEY_BYTES_LENGTH):
    """The symmetric key of 16-bit ``pattern``: ``pattern >> 8, pattern & 0xFF`` repeated over
    ``length`` bytes (``symmetric_key(0x6d5a)`` is DPDK's ``6d:5a:6d:5a:...``)."""
    return _native.symmetric_key(pattern, length)


SYMMETRIC_CHUNK_BYTES = 256 << 20  # one scan's loads in symmetric_search


def _pattern_range(patterns):
    if patterns is None:
        return 0, _native.SYMMETRIC_PATTERNS
    if isinstance(patterns, range):
        if patterns.step != 1:
            raise ValueError("patterns must be consecutive, got %r" % (patterns,))
        return patterns.start, len(patterns)
    first, count = patterns
    return int(first), int(count)


def symmetric_loads(tuples, htable, nqueues, patterns=None, ipv6=False, weights=None,
                    fields=_native.FIELDS_ALL, ctx=None):
    """uint64 loads ``[npatterns, min(H, Q)]`` of packed ``tuples`` under the symmetric keys of
    ``patterns`` (a ``range`` or ``(first, count)``; default all 65536): row r is the per-queue
    flow counts -- with ``weights`` (one u32 per tuple) the loads -- under
    ``symmetric_key(first + r)`` (GPU: one fold of the flows, one scan of the patterns).
    ``ipv6``: ``TUPLE6_DTYPE`` or ``(n, 9)`` uint32 tuples; ``fields``: the hashed fields, a
    mask or 'sdfn' letters."""
    first, count = _pattern_range(patterns)
    ctx = ctx or _native.default_context()
    return ctx.symmetric_search(tuples, htable, nqueues, first, count, ipv6, weights, fields)


def symmetric_search(tuples, htable, nqueues, patterns=None, ipv6=False, weights=None,
                     fields=_native.FIELDS_ALL, top=10):
    """Rank the symmetric keys of ``patterns`` (default all 65536) for ``tuples`` with
    :func:`balance`, exhaustively; the range is scanned in chunks whose loads stay at or below
    256 MiB.  Returns dicts like :func:`search` (best first) plus ``"pattern"``."""
    first, count = _pattern_range(patterns)
    width = _native.queue_modulus(htable, nqueues)[1]
    chunk = max(1, SYMMETRIC_CHUNK_BYTES // (8 * width))
    best = []  # (max_load, chi2, pattern, used, counts)
    for start in range(first, first + count, chunk):
        loads = symmetric_loads(tuples, htable, nqueues, (start, min(chunk, first + count - start)),
                                ipv6, weights, fields)
        m = balance(loads, htable, nqueues)
        for i in np.lexsort((m["chi2"], m["max_load"]))[:top]:
            best.append((float(m["max_load"][i]), float(m["chi2"][i]), start + int(i),
                         int(m["used"][i]), loads[i].copy()))
        best = sorted(best, key=lambda r: r[:3])[:top]
    return [{"key": symmetric_key(p), "pattern": p, "max_load": ml, "chi2": chi2, "used": used,
             "counts": counts} for ml, chi2, p, used, counts in best]


def flip_bit(key, j):
    """``key`` with bit ``j`` flipped (0 = MSB of byte 0), as a new list."""
    out = [int(b) for b in key]
    out[j >> 3] ^= 0x80 >> (j & 7)
    return out


def neighbourhood(key, tuples, htable, nqueues, ctx=None, ipv6=False, weights=None):
    """uint64 counts ``[128, min(H, Q)]`` of packed ``tuples`` under every single-bit flip of
    ``key`` (GPU, one launch): row j = ``flip_bit(key, j)``; key bit 127 feeds no IPv4 hash,
    so row 127 is ``key`` itself.  ``ipv6``: 320 rows over IPv6 tuples, row 319 the key itself.
    ``weights`` (IPv4 only): the rows are loads, the sums of the tuples' weights."""
    _no_ipv6_weights(ipv6, weights)
    ctx = ctx or _native.default_context()
    if ipv6:
        return ctx.key_neighbourhood6(_native.prepare_key6(key), tuples, htable, nqueues)
    if weights is None:
        return ctx.key_neighbourhood(_native.prepare_key(key), tuples, htable, nqueues)
    return ctx.key_neighbourhood(_native.prepare_key(key), tuples, htable, nqueues,
                                 weights=weights)


def _resident_neighbourhood(tuples, htable, nqueues, ipv6=False, weights=None):
    """``key -> counts[128, min(H, Q)]`` (``ipv6``: 320 rows) on tuples uploaded once: one
    ``rss_key_neighbourhood_device`` / ``rss_key_neighbourhood6_device`` launch per call; with
    ``weights``, uploaded once beside the tuples, ``rss_key_neighbourhood_weighted_device``."""
    _no_ipv6_weights(ipv6, weights)
    import torch
    arr = np.ascontiguousarray(tuples)
    if arr.dtype != (_native.TUPLE6_DTYPE if ipv6 else _native.TUPLE_DTYPE):
        arr = np.ascontiguousarray(arr, dtype=np.uint32).reshape(-1, 9 if ipv6 else 3)
    n = len(arr)
    dev = torch.device("cuda:%d" % _native.default_context().device)
    flat = np.ascontiguousarray(arr).view(np.int32).reshape(-1)
    d_tuples = torch.from_numpy(flat).to(dev)
    if weights is not None:
        d_weights = torch.from_numpy(_native.tuple_weights(weights, n).view(np.int32)).to(dev)
    width = _native.queue_modulus(htable, nqueues)[1]
    rows = _native.KEY6_NEIGHBOURS if ipv6 else _native.KEY_NEIGHBOURS
    d_counts = torch.empty((rows, width), dtype=torch.int64, device=dev)

    def score(key):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if ipv6:
            _native.key_neighbourhood6_device(_native.prepare_key6(key), d_tuples.data_ptr(), n,
                                              htable, nqueues, d_counts.data_ptr(), stream)
        elif weights is not None:
            _native.key_neighbourhood_weighted_device(
                _native.prepare_key(key), d_tuples.data_ptr(), d_weights.data_ptr(), n, htable,
                nqueues, d_counts.data_ptr(), stream)
        else:
            _native.key_neighbourhood_device(_native.prepare_key(key), d_tuples.data_ptr(), n,
                                             htable, nqueues, d_counts.data_ptr(), stream)
        return d_counts.cpu().numpy().view(np.uint64)

    return score


def _byte_range(bytes, ipv6):
    total = _native.KEY6_BYTES if ipv6 else _native.KEY_BYTES
    if bytes is None:
        return 0, total
    if isinstance(bytes, range):
        if bytes.step != 1:
            raise ValueError("bytes must be consecutive, got %r" % (bytes,))
        return bytes.start, len(bytes)
    first, count = bytes
    return int(first), int(count)


def byte_neighbourhood(key, tuples, htable, nqueues, bytes=None, ctx=None, ipv6=False,
                       weights=None):
    """uint64 counts ``[nbytes * 256, min(H, Q)]`` of packed ``tuples`` under every value of
    every key byte in ``bytes`` (a ``range`` with step 1 or ``(first, count)``; default all 16,
    ``ipv6``: 40) -- GPU, one launch: row ``256 * (B - first) + v`` = ``key`` with byte B set
    to v, so row ``256 * (B - first) + key[B]`` is ``key`` itself.  ``weights`` (IPv4 only):
    the rows are loads, the sums of the tuples' weights."""
    _no_ipv6_weights(ipv6, weights)
    first, count = _byte_range(bytes, ipv6)
    ctx = ctx or _native.default_context()
    if ipv6:
        return ctx.key_byte_neighbourhood6(_native.prepare_key6(key), tuples, htable, nqueues,
                                           first, count)
    return ctx.key_byte_neighbourhood(_native.prepare_key(key), tuples, htable, nqueues, first,
                                      count, weights)


def _resident_byte_neighbourhood(tuples, htable, nqueues, ipv6=False, weights=None):
    """``key -> counts[16 * 256, min(H, Q)]`` (``ipv6``: 40 * 256 rows) on tuples -- and
    ``weights`` -- uploaded once: one ``rss_key_byte_neighbourhood_device`` / ``..6_device`` /
    ``.._weighted_device`` launch per call."""
    _no_ipv6_weights(ipv6, weights)
    import torch
    arr = np.ascontiguousarray(tuples)
    if arr.dtype != (_native.TUPLE6_DTYPE if ipv6 else _native.TUPLE_DTYPE):
        arr = np.ascontiguousarray(arr, dtype=np.uint32).reshape(-1, 9 if ipv6 else 3)
    n = len(arr)
    dev = torch.device("cuda:%d" % _native.default_context().device)
    d_tuples = torch.from_numpy(np.ascontiguousarray(arr).view(np.int32).reshape(-1)).to(dev)
    if weights is not None:
        d_weights = torch.from_numpy(_native.tuple_weights(weights, n).view(np.int32)).to(dev)
    width = _native.queue_modulus(htable, nqueues)[1]
    nbytes = _native.KEY6_BYTES if ipv6 else _native.KEY_BYTES
    d_counts = torch.empty((nbytes * 256, width), dtype=torch.int64, device=dev)

    def score(key):
        stream = torch.cuda.current_stream(dev).cuda_stream
        if ipv6:
            _native.key_byte_neighbourhood6_device(
                _native.prepare_key6(key), 0, nbytes, d_tuples.data_ptr(), n, htable, nqueues,
                d_counts.data_ptr(), stream)
        elif weights is not None:
            _native.key_byte_neighbourhood_weighted_device(
                _native.prepare_key(key), 0, nbytes, d_tuples.data_ptr(), d_weights.data_ptr(), n,
                htable, nqueues, d_counts.data_ptr(), stream)
        else:
            _native.key_byte_neighbourhood_device(
                _native.prepare_key(key), 0, nbytes, d_tuples.data_ptr(), n, htable, nqueues,
                d_counts.data_ptr(), stream)
        return d_counts.cpu().numpy().view(np.uint64)

    return score


def _refine_bytes(key, score, htable, nqueues, max_steps):
    """:func:`refine` with ``step="byte"``: coordinate descent over the key's bytes."""
    moves = []
    counts = np.asarray(score(key))
    while True:
        own = key[0]  # row 256 * 0 + key[0]: the key's own counts
        m = balance(counts, htable, nqueues)
        best = int(np.lexsort((m["chi2"], m["max_load"]))[0])
        better = (m["max_load"][best], m["chi2"][best]) < (m["max_load"][own], m["chi2"][own])
        if not better or len(moves) >= max_steps:
            return {"key": key, "max_load": float(m["max_load"][own]), "chi2": float(m["chi2"][own]),
                    "used": int(m["used"][own]), "counts": counts[own].copy(), "flips": [],
                    "moves": moves}
        key = list(key)
        key[best >> 8] = best & 0xFF
        moves.append((best >> 8, best & 0xFF))
        counts = np.asarray(score(key))


def refine(key, tuples, htable, nqueues, max_steps=64, neighbourhood=None, ipv6=False,
           weights=None, step="bit"):
    """Hill-climb ``key`` over single-bit flips (steepest descent on ``(max_load, chi2)``).

    Each step scores the key's 128 neighbours (``ipv6``: 320; one
    ``rss_key_neighbourhood_device`` / ``rss_key_neighbourhood6_device`` launch on tuples
    uploaded once; or ``neighbourhood(key) -> counts[rows, Q]`` when given) with
    :func:`balance` and flips the bit whose row has the lexicographically smallest
    ``(max_load, chi2)``, as long as that is strictly below the key's own (the last row); it stops
    at a local optimum or after ``max_steps`` flips.  Returns a dict: ``key``, ``max_load``,
    ``chi2``, ``used``, ``counts`` (of the returned key) and ``flips`` (the bits, in order).
    With ``weights`` (IPv4 only; uploaded once beside the tuples,
    ``rss_key_neighbourhood_weighted_device``) the climb is on per-queue loads.

    ``step="byte"`` descends over whole bytes instead: each step scores every value of every
    key byte (16 * 256 rows, ``ipv6``: 40 * 256; one ``rss_key_byte_neighbourhood_device`` /
    ``..6_device`` / ``.._weighted_device`` launch, or ``neighbourhood(key)`` returning those
    rows) and sets the byte of the smallest ``(max_load, chi2)`` row while that is strictly
    below the key's own (row ``key[0]``).  A byte's values contain its single-bit flips, so one
    byte step is never worse than one bit step.  The dict then holds ``moves``, the ``(byte,
    value)`` pairs in order, and an empty ``flips``.
    """
    _no_ipv6_weights(ipv6, weights)
    if step not in ("bit", "byte"):
        raise ValueError("step must be 'bit' or 'byte', got %r" % (step,))
    key = [int(b) for b in key]
    if step == "byte":
        score = neighbourhood or _resident_byte_neighbourhood(tuples, htable, nqueues, ipv6,
                                                              weights)
        return _refine_bytes(key, score, htable, nqueues, max_steps)
    score = neighbourhood or _resident_neighbourhood(tuples, htable, nqueues, ipv6, weights)
    flips = []
    counts = np.asarray(score(key))
    while True:
        own = len(counts) - 1  # the last key bit feeds no hash: the key's own counts
        m = balance(counts, htable, nqueues)
        best = int(np.lexsort((m["chi2"], m["max_load"]))[0])
        better = (m["max_load"][best], m["chi2"][best]) < (m["max_load"][own], m["chi2"][own])
        if not better or len(flips) >= max_steps:
            return {"key": key, "max_load": float(m["max_load"][own]), "chi2": float(m["chi2"][own]),
                    "used": int(m["used"][own]), "counts": counts[own].copy(), "flips": flips}
        key = flip_bit(key, best)
        flips.append(best)
        counts = np.asarray(score(key))


def load_tuples(ips_file, ipv6=False):
    """Packed tuples of a 4-tuple CSV: native fast path, else the pandas ingest."""
    data = np.fromfile(ips_file, dtype=np.uint8)
    parsed = _native.csv_parse6(data) if ipv6 else _native.csv_parse(data)
    if parsed is not None:
        return parsed[0]
    return (pack_frame6 if ipv6 else pack_frame)(pd.read_csv(ips_file))


def load_weighted_csv(ips_file, column):
    """``(tuples, weights)`` of a 4-tuple CSV with a ``column`` of per-flow weights, read
    through pandas; ``ValueError`` unless the column holds integers in [0, 2^32)."""
    df = pd.read_csv(ips_file)
    if column not in df.columns:
        raise ValueError("%s has no column %r" % (ips_file, column))
    return pack_frame(df), _native.tuple_weights(df[column].to_numpy(), len(df))


def load_timed_csv(ips_file, time_column, width, weight_column=None):
    """``(tuples, weights, slots, nslots)`` of a CSV with one row per packet: the packed
    tuples, the ``weight_column`` (or None), and each packet's window from the numeric
    ``time_column`` (:func:`window_slots`).  ``ValueError`` for a missing column or bad values."""
    df = pd.read_csv(ips_file)
    for column in (time_column, weight_column):
        if column is not None and column not in df.columns:
            raise ValueError("%s has no column %r" % (ips_file, column))
    if df[time_column].dtype.kind not in "iuf":
        raise ValueError("column %r of %s is not numeric" % (time_column, ips_file))
    slots, nslots = window_slots(df[time_column].to_numpy(), width)
    weights = None
    if weight_column is not None:
        weights = _native.tuple_weights(df[weight_column].to_numpy(), len(df))
    return pack_frame(df), weights, slots, nslots


def load_ticks(ips_file, time_column, width):
    """Each row's arrival tick of :func:`load_timed_csv`'s CSV: ``window_slots(times, width)[0]``."""
    return window_slots(pd.read_csv(ips_file, usecols=[time_column])[time_column].to_numpy(),
                        width)[0]


def load_weighted_csv6(ips_file, column):
    """:func:`load_weighted_csv` for a CSV of IPv6 flows (``TUPLE6_DTYPE`` tuples)."""
    df = pd.read_csv(ips_file)
    if column not in df.columns:
        raise ValueError("%s has no column %r" % (ips_file, column))
    return pack_frame6(df), _native.tuple_weights(df[column].to_numpy(), len(df))


def _score_given_symmetric(key, tuples, htable, nqueues, ipv6, weights):
    """``--symmetric``: the ``--key-file`` key's loads.  The hash entries serve any key, IPv4 or
    IPv6; weighted, the key is one more candidate of the weighted search (IPv4), and an IPv6
    key's loads are its queues' weights summed on the host."""
    if weights is None or not ipv6:
        return evaluate([key], tuples, htable, nqueues, ipv6=ipv6, weights=weights)
    from rss_simulator_nvidia_amd.toeplitz import Toeplitz
    _, queues, counts = Toeplitz(key).compute_queues6(tuples, htable, nqueues)
    loads = np.zeros(len(counts), dtype=np.uint64)
    np.add.at(loads, queues, weights.astype(np.uint64))
    return loads[None, :_native.queue_modulus(htable, nqueues)[1]]


def main(argv=None):
    p = argparse.ArgumentParser(prog="rss-keysearch", description=__doc__.splitlines()[0])
    source = p.add_mutually_exclusive_group(required=True)
    source.add_argument("--ips-file", metavar="PATH")
    source.add_argument("--pcap", metavar="PATH",
                        help="a capture instead of a CSV: its unique IPv4 flows, each weighted "
                             "by its packets, so that the printed max_load, chi2 and queues used "
                             "describe the packet load per queue, not the flow count")
    p.add_argument("--weight-column", metavar="NAME",
                   help="CSV column of per-flow weights (packets or bytes: integers in "
                        "[0, 2^32)); the printed max_load, chi2 and queues used then describe "
                        "the load per queue, not the flow count")
    p.add_argument("--htable-size", metavar="NUM", type=PositiveInt.parse, required=True)
    p.add_argument("--num-queues", metavar="NUM", type=PositiveInt.parse, required=True)
    p.add_argument("--keys", metavar="NUM", type=PositiveInt.parse, default=1024,
                   help="random candidate keys to evaluate (unused with --symmetric)")
    p.add_argument("--seed", type=int, default=0, help="of the random candidates (unused with "
                                                       "--symmetric)")
    p.add_argument("--top", metavar="NUM", type=PositiveInt.parse, default=5)
    p.add_argument("--key-file", metavar="PATH", dest="key",
                   type=apt_decorator(HashKey.from_file),
                   help="also score this key (e.g. the one in use)")
    p.add_argument("--refine", metavar="STEPS", type=int, default=0,
                   help="then hill-climb the top-ranked key (and the --key-file key) over "
                        "single-bit flips, at most STEPS flips each")
    p.add_argument("--refine-step", choices=("bit", "byte"), default="bit",
                   help="what one --refine step changes: the best single bit (default), or the "
                        "best value of any one key byte (every value of every byte is scored per "
                        "step)")
    p.add_argument("--out", metavar="PATH", help="write the best key in --key-file format")
    p.add_argument("--ipv6", action="store_true",
                   help="the file holds IPv6 flows (36-byte hash input, 320 key bits)")
    p.add_argument("--symmetric", action="store_true",
                   help="rank all 65536 symmetric keys (a 16-bit pattern repeated, like DPDK's "
                        "6d:5a:...) instead of random candidates: both directions of a "
                        "connection share a queue; exhaustive, IPv4 or IPv6, weighted or not")
    p.add_argument("--aggregate", action="store_true",
                   help="the CSV holds one row per packet: fold the rows to flows (on the GPU) "
                        "and rank by load, the sum of --weight-column per flow or the rows per "
                        "flow without it")
    p.add_argument("--time-column", metavar="NAME",
                   help="the CSV holds one row per packet and NAME is its numeric time: after "
                        "the ranking, print each listed key's peak -- its hottest queue in any "
                        "window of --window, relative to the busiest window's ideal share")
    p.add_argument("--window", metavar="WIDTH", type=float,
                   help="width of a time window, in the units of --time-column")
    p.add_argument("--drain", metavar="UNITS", type=int,
                   help="with --tick: also print each listed key's peak backlog, every queue "
                        "draining UNITS of load (packets, or --weight-column units) per tick")
    p.add_argument("--tick", metavar="WIDTH", type=float,
                   help="width of a --drain tick, in the units of --time-column")
    args = p.parse_args(argv)
    if (args.drain is None) != (args.tick is None):
        p.error("--drain and --tick go together: a queue drains --drain units per --tick")
    if args.drain is not None and args.time_column is None:
        p.error("--drain and --tick need --time-column (and --window): the backlog takes the "
                "rows in time order")
    if args.drain is not None and not 0 <= args.drain < 2**31:
        p.error("--drain must be an integer in [0, 2^31), got %r" % args.drain)
    if args.tick is not None and not args.tick > 0:
        p.error("--tick must be > 0, got %r" % args.tick)
    if (args.time_column is None) != (args.window is None):
        p.error("--time-column and --window go together: the column holds each packet's time, "
                "the width cuts it into windows")
    if args.time_column and (args.pcap or args.ipv6 or args.aggregate):
        p.error("--time-column cannot be combined with --pcap, --ipv6 or --aggregate: the "
                "timeline takes the rows of an IPv4 CSV as packets")
    if args.window is not None and not args.window > 0:
        p.error("--window must be > 0, got %r" % args.window)
    if args.aggregate and args.pcap:
        p.error("--aggregate folds the rows of a CSV: not allowed with --pcap, whose packets "
                "are always folded to flows")
    if args.symmetric and args.refine > 0:
        p.error("--refine cannot be combined with --symmetric: a single-bit flip breaks the "
                "key's symmetry")
    if args.symmetric and args.refine_step != "bit":
        p.error("--refine-step cannot be combined with --symmetric: a changed byte breaks the "
                "key's symmetry")
    if args.refine > 0:
        # refine keeps its tuples in torch tensors: torch opens the device before the
        # library's first call does (the other order leaves torch without a device)
        import torch
        torch.cuda.init()
    weights = None
    if args.ipv6 and (args.pcap or args.weight_column or args.aggregate) and not args.symmetric:
        p.error("--ipv6 cannot be combined with --pcap or --weight-column: weighted key "
                "search serves IPv4 flows only")
    if args.pcap and args.weight_column:
        p.error("--weight-column names a CSV column: not allowed with --pcap")
    slots = None
    if args.pcap:
        from rss_simulator_nvidia_amd.pcap import read_flows
        tuples, _, _, weights = read_flows(args.pcap, ipv6=args.ipv6, packet_counts=True,
                                           on_device=True)
    elif args.time_column:
        try:
            tuples, weights, slots, nslots = load_timed_csv(args.ips_file, args.time_column,
                                                            args.window, args.weight_column)
        except ValueError as err:
            p.error("--time-column %s: %s" % (args.time_column, err))
    elif args.weight_column:
        try:
            tuples, weights = (load_weighted_csv6 if args.ipv6 else load_weighted_csv)(
                args.ips_file, args.weight_column)
        except ValueError as err:
            p.error("--weight-column %s: %s" % (args.weight_column, err))
    else:
        tuples = load_tuples(args.ips_file, args.ipv6)
    if args.aggregate:
        from rss_simulator_nvidia_amd.flows import aggregate
        tuples, loads, _ = aggregate(tuples, weights, args.ipv6)
        try:
            weights = _native.tuple_weights(loads, len(loads))  # the weighted search takes u32
        except ValueError as err:
            p.error("--aggregate: a flow's summed weight: %s" % err)
    extra = [args.key] if args.key else []
    if args.symmetric:
        ranked = symmetric_search(tuples, args.htable_size, args.num_queues, ipv6=args.ipv6,
                                  weights=weights, top=args.top)
    else:
        ranked = search(tuples, args.htable_size, args.num_queues, args.keys, args.seed, args.top,
                        extra, args.ipv6, weights)
    if args.key:
        given = (_score_given_symmetric(args.key, tuples, args.htable_size, args.num_queues,
                                        args.ipv6, weights) if args.symmetric else
                 evaluate([args.key], tuples, args.htable_size, args.num_queues,
                          ipv6=args.ipv6, weights=weights))
        base = balance(given, args.htable_size, args.num_queues)
        print("given key: max_load %.4f chi2 %.2f queues used %d"
              % (base["max_load"][0], base["chi2"][0], base["used"][0]))
    for r in ranked:
        print("%s  max_load %.4f chi2 %.2f queues used %d"
              % (key_text(r["key"]), r["max_load"], r["chi2"], r["used"]))
    if args.refine > 0:
        starts = [ranked[0]["key"]] + extra
        resident = (_resident_byte_neighbourhood if args.refine_step == "byte"
                    else _resident_neighbourhood)
        score = resident(tuples, args.htable_size, args.num_queues, args.ipv6, weights)
        refined = [refine(k, tuples, args.htable_size, args.num_queues, args.refine, score,
                          step=args.refine_step) for k in starts]
        refined.sort(key=lambda r: (r["max_load"], r["chi2"]))
        for r in refined:
            print("%s  max_load %.4f chi2 %.2f queues used %d"
                  % (key_text(r["key"]), r["max_load"], r["chi2"], r["used"]))
        ranked = refined + ranked  # --out takes the best refined key
    if slots is not None:  # one timeline launch over every key listed above
        listed = []
        for key in [list(k) for k in extra] + [list(r["key"]) for r in ranked]:
            if key not in listed:
                listed.append(key)
        pk = peak(timeline(listed, tuples, slots, args.htable_size, args.num_queues, nslots,
                           weights), args.htable_size, args.num_queues)
        for key, value, window in zip(listed, pk["peak"], pk["window"]):
            print("%s  peak %.4f at window %d of %d" % (key_text(key), value, window, nslots))
        if args.drain is not None:  # the rows in tick order, for this call only
            try:
                ticks = load_ticks(args.ips_file, args.time_column, args.tick)
            except ValueError as err:
                p.error("--tick %r: %s" % (args.tick, err))
            order = np.argsort(ticks, kind="stable")
            peaks = backlog(listed, tuples[order], ticks[order], args.drain, args.htable_size,
                            args.num_queues, None if weights is None else weights[order])
            for key, row in zip(listed, peaks):
                print("%s  backlog %d at queue %d" % (key_text(key), row.max(), row.argmax()))
    if args.out:
        with open(args.out, "w") as f:
            f.write(key_text(ranked[0]["key"]))
    return ranked


if __name__ == "__main__":
    main()
