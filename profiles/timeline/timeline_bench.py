"""Times of rss_key_search_timeline_device on one MI355X (writes times.json beside itself, or
to --out): 2^26 resident time-ordered packets with u32 weights, H = 128, Q in {24, 64}, 8 and
64 keys, W in {64, 1024, 16384} windows of equal length, event-timed after a warm-up launch.

Per configuration:
  timeline           the new entry on the ordered packets
  timeline_permuted  the same packets in a random permutation (the slow case; compared equal)
  per_window         baseline (a): W launches of rss_key_search_weighted_device over the W
                     contiguous slices (loads compared equal to the timeline's)
  wq_queues          baseline (b): one rss_key_search_weighted_device launch with htable =
                     nqueues = W * Q.  The existing entry takes a queue from the tuple alone, so
                     it cannot produce per-window loads; this is the launch such a variant would
                     cost at best -- one global atomic per (packet, key) over W * Q bins, spread
                     by the hash instead of piling on the current window's Q.  Not compared.
`stream_fraction` is the time the tuple + weight + slot bytes (20 B a packet) take at 8 TB/s
over the measured time; `lds_model_ms` is arithmetic, not a counter: 21 ds_read_b64 per packet
and key group plus one 8-byte LDS atomic (counted twice: read and write) per packet and key,
at 128 B per clock and CU, 256 CUs, 2.4 GHz.

    python profiles/timeline/timeline_bench.py [--log2n 26] [--out PATH]
"""
import argparse
import json
import os
import statistics

import numpy as np
import torch

from rss_simulator_nvidia_amd import _native, keysearch

HBM_BYTES_PER_S = 8e12
LDS_BYTES_PER_S = 256 * 128 * 2.4e9
H = 128


def timed(fn, budget_s=1.0):
    """Median / min / max ms of `fn` over 2..20 event-timed launches after one warm-up."""
    fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = []
    while len(times) < 2 or (len(times) < 20 and sum(times) < budget_s * 1e3):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times),
            "reps": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=26)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                  "times.json"))
    args = ap.parse_args()
    n = 1 << args.log2n
    dev = torch.device("cuda:0")
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    d_t = torch.empty(3 * n, dtype=torch.int32, device=dev)
    _native.generate_device(7, 0, n, d_t.data_ptr(), stream())
    d_w = torch.randint(-2**31, 2**31, (n,), dtype=torch.int32, device=dev)  # any u32 bit pattern
    perm = torch.randperm(n, device=dev)
    p_t = d_t.view(n, 3)[perm].contiguous().view(-1)
    p_w = d_w[perm].contiguous()
    results = []
    for nkeys in (8, 64):
        keys = keysearch.random_keys(nkeys, seed=nkeys)
        win = np.stack([np.ctypeslib.as_array(_native.prepare_key(k).window) for k in keys])
        d_win = torch.from_numpy(win.astype(np.uint32).view(np.int32)).to(dev)
        for Q in (24, 64):
            for W in (64, 1024, 16384):
                d_s = (torch.arange(n, dtype=torch.int64, device=dev) * W // n).to(torch.int32)
                p_s = d_s[perm].contiguous()
                loads = torch.empty((nkeys, W, Q), dtype=torch.int64, device=dev)
                other = torch.empty((nkeys, W, Q), dtype=torch.int64, device=dev)
                row = {"n": n, "H": H, "Q": Q, "keys": nkeys, "windows": W}
                row["timeline"] = timed(lambda: _native.key_search_timeline_device(
                    d_win.data_ptr(), nkeys, d_t.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), n, W,
                    H, Q, loads.data_ptr(), stream()))
                row["timeline_permuted"] = timed(lambda: _native.key_search_timeline_device(
                    d_win.data_ptr(), nkeys, p_t.data_ptr(), p_w.data_ptr(), p_s.data_ptr(), n, W,
                    H, Q, other.data_ptr(), stream()))
                row["permuted_equal"] = bool(torch.equal(loads, other))
                per = n // W  # equal windows: slice s is packets [s * per, (s + 1) * per)
                sliced = torch.empty((W, nkeys, Q), dtype=torch.int64, device=dev)

                def per_window():
                    for s in range(W):
                        _native.key_search_weighted_device(
                            d_win.data_ptr(), nkeys, d_t.data_ptr() + 12 * s * per,
                            d_w.data_ptr() + 4 * s * per, per, H, Q, sliced[s].data_ptr(), stream())
                row["per_window"] = timed(per_window)
                row["per_window_equal"] = bool(torch.equal(loads, sliced.permute(1, 0, 2)))
                del sliced
                wide = torch.empty((nkeys, W * Q), dtype=torch.int64, device=dev)
                row["wq_queues"] = timed(lambda: _native.key_search_weighted_device(
                    d_win.data_ptr(), nkeys, d_t.data_ptr(), d_w.data_ptr(), n, W * Q, W * Q,
                    wide.data_ptr(), stream()))
                del wide
                floor_ms = 20.0 * n / HBM_BYTES_PER_S * 1e3
                for name in ("timeline", "timeline_permuted", "per_window", "wq_queues"):
                    row[name]["stream_fraction"] = floor_ms / row[name]["median_ms"]
                groups = -(-nkeys // (8 if Q <= 38 else 4))  # keys per workgroup at H = 128
                row["stream_floor_ms"] = floor_ms
                row["lds_model_ms"] = n * (groups * 21 * 8 + nkeys * 16) / LDS_BYTES_PER_S * 1e3
                row["per_window_over_timeline"] = (row["per_window"]["median_ms"]
                                                   / row["timeline"]["median_ms"])
                row["wq_queues_over_timeline"] = (row["wq_queues"]["median_ms"]
                                                  / row["timeline"]["median_ms"])
                row["permuted_over_ordered"] = (row["timeline_permuted"]["median_ms"]
                                                / row["timeline"]["median_ms"])
                results.append(row)
                print(json.dumps(row), flush=True)
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
