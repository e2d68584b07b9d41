"""Packets to flows on the GPU (``rss_flow_aggregate_host``): the distinct tuples of a packet
list in first-seen order, each with its load -- the sum of a per-packet weight, or its packet
count -- and the index of its first packet.  The flows and loads are what ``keysearch``'s
weighted ranking takes; ``pcap.read_flows(on_device=True)`` and ``keysearch --aggregate`` go
through here."""
import numpy as np

from rss_simulator_nvidia_amd import _native


def aggregate(tuples, weights=None, ipv6=False, ctx=None):
    """``(flows, loads, first)`` of packed ``tuples`` (``TUPLE_DTYPE``, ``ipv6``:
    ``TUPLE6_DTYPE``, or ``(n, 3)`` / ``(n, 9)`` uint32): ``flows`` the distinct tuples in
    first-seen order with the input's dtype, ``loads`` uint64 sums of ``weights`` (one integer
    in [0, 2^32) per packet; 1 each without), ``first`` uint32 indices of the flows' first
    packets."""
    ctx = ctx or _native.default_context()
    arr = np.asarray(tuples)
    flows, loads, first = ctx.aggregate_flows(arr, weights, ipv6)
    record = _native.TUPLE6_DTYPE if ipv6 else _native.TUPLE_DTYPE
    if arr.dtype == record:
        flows = flows.view(record).reshape(-1)
    elif arr.dtype != np.uint32:
        flows = flows.astype(arr.dtype)
    return flows, loads, first
