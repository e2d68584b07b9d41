"""Times of rss_key_search_backlog_device on one MI355X (writes times.json beside itself, or to
--out): resident time-ordered packets with u32 weights (below 2^16, so that the drain fits), H =
128, Q in {24, 64}, 8 and 64 keys, 2^24 and 2^26 packets, event-timed after a warm-up launch.
Ticks: 1024 per capture (packet i at tick i * 1024 // n); drain: the mean weight times the
packets per tick over Q, so that queues hover around empty and backlogs cross many segments.

Per configuration:
  backlog    the new entry (both kernels)
  timeline   comparison (a): one rss_key_search_timeline_device launch over the same packets and
             keys with the ticks as slots of 1024 windows -- the same stream, the same hashing; a
             floor, not a target
  host_route comparison (b): what the entry replaces, per key: one rss_hash_device launch for
             the queue column, the column copied to the host, and numpy's form of the recurrence
             per queue.  Timed once for one key (it takes seconds) and its peaks compared equal to
             the entry's; `host_route_ms` is that time x keys, which is how the route scales.
`segments` repeats the launcher's rule (rss_backlog.hip) for this device's CU count.
`scan_model_ms` is arithmetic, not a counter: 25 VALU instructions per (lane, packet) of the
scan, each 4 clocks of a SIMD for a wave of 64, 16 waves on 4 SIMDs, S packets (one per segment)
a step, 256 CUs at 2.4 GHz, once per key group.

    python profiles/backlog/backlog_bench.py [--log2n 24 26] [--out PATH] [--only-backlog]

--only-backlog runs the entry alone a few times per configuration: the run to put under a
kernel trace for the two kernels' separate times (kernels.json here came from one).
"""
import argparse
import json
import os
import statistics
import time

import numpy as np
import torch

from rss_simulator_nvidia_amd import _native, keysearch

H, TICKS = 128, 1024


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


def segments(n, nkeys, Q, cus):
    """(segments, segments per workgroup, keys per workgroup) of the launcher at H = 128."""
    keys = 8 if nkeys > 4 and Q <= 128 else 4 if nkeys > 1 else 1
    per_wg = min(16, 1024 // (keys * Q))
    groups = -(-nkeys // keys)
    want = min(8192, per_wg * max(1, 2 * cus // groups))
    seg_len = max(256, -(-n // want))
    return -(-n // seg_len), per_wg, keys


def host_route(key, d_t, w, ticks, n, Q, drain, stream):
    """Comparison (b) for one key: (ms, peaks)."""
    d_q = torch.empty(n, dtype=torch.int32, device=d_t.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _native.hash_device(_native.prepare_key(key), d_t.data_ptr(), n, H, Q,
                        queue_ptr=d_q.data_ptr(), stream=stream)
    queues = d_q.cpu().numpy()
    peaks = np.zeros(Q, dtype=np.uint64)
    a_all = np.int64(drain) * ticks
    for q in range(Q):
        idx = queues == q
        if idx.any():
            wq, a = w[idx], a_all[idx]
            S = np.cumsum(wq)
            peaks[q] = (S + np.maximum.accumulate(a - (S - wq)) - a).max()
    return (time.perf_counter() - t0) * 1e3, peaks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, nargs="+", default=[24, 26])
    ap.add_argument("--only-backlog", action="store_true")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                                  "times.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    results = []
    for log2n in args.log2n:
        n = 1 << log2n
        d_t = torch.empty(3 * n, dtype=torch.int32, device=dev)
        _native.generate_device(7, 0, n, d_t.data_ptr(), stream())
        d_w = torch.randint(0, 2**16, (n,), dtype=torch.int32, device=dev)
        d_s = (torch.arange(n, dtype=torch.int64, device=dev) * TICKS // n).to(torch.int32)
        w = d_w.cpu().numpy().view(np.uint32).astype(np.int64)
        ticks = d_s.cpu().numpy().astype(np.int64)
        for Q in (24, 64):
            drain = min(int(w.mean() * (n // TICKS) / Q), 2**31 - 1)
            for nkeys in (8, 64):
                keys = keysearch.random_keys(nkeys, seed=nkeys)
                win = np.stack([np.ctypeslib.as_array(_native.prepare_key(k).window) for k in keys])
                d_win = torch.from_numpy(win.astype(np.uint32).view(np.int32)).to(dev)
                need = _native.key_search_backlog_workspace_bytes(nkeys, n, H, Q)
                ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
                peaks = torch.empty((nkeys, Q), dtype=torch.int64, device=dev)
                nseg, per_wg, per_group = segments(n, nkeys, Q, cus)
                row = {"n": n, "H": H, "Q": Q, "keys": nkeys, "drain": drain, "cus": cus,
                       "segments": nseg, "segments_per_workgroup": per_wg,
                       "workspace_bytes": need}
                row["backlog"] = timed(lambda: _native.key_search_backlog_device(
                    d_win.data_ptr(), nkeys, d_t.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), n,
                    drain, H, Q, peaks.data_ptr(), ws.data_ptr(), need, stream()))
                groups = -(-nkeys // per_group)
                row["scan_model_ms"] = (n / per_wg * 25 * 4 * 4 * groups) / (cus * 2.4e9) * 1e3
                if not args.only_backlog:
                    loads = torch.empty((nkeys, TICKS, Q), dtype=torch.int64, device=dev)
                    row["timeline"] = timed(lambda: _native.key_search_timeline_device(
                        d_win.data_ptr(), nkeys, d_t.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), n,
                        TICKS, H, Q, loads.data_ptr(), stream()))
                    del loads
                    ms, ref = host_route(keys[0], d_t, w, ticks, n, Q, drain, stream())
                    row["host_route_one_key_ms"] = ms
                    row["host_route_ms"] = ms * nkeys
                    row["host_route_equal"] = bool(
                        (peaks[0].cpu().numpy().view(np.uint64) == ref).all())
                    row["backlog_over_timeline"] = (row["backlog"]["median_ms"]
                                                    / row["timeline"]["median_ms"])
                    row["host_route_over_backlog"] = row["host_route_ms"] / row["backlog"]["median_ms"]
                results.append(row)
                print(json.dumps(row), flush=True)
                with open(args.out, "w") as f:
                    json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
