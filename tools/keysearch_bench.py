"""Key-search throughput (tool, not product): K random keys x n resident flows, one launch.
Prints key-tuple evaluations per second.
usage: python tools/keysearch_bench.py [K] [n] [uniform|flow] [H] [Q]
       python tools/keysearch_bench.py neighbourhood [n] [uniform|flow] [H] [Q]
The neighbourhood mode times one rss_key_neighbourhood_device launch (the 128 single-bit
flips of one key) against the same job as one rss_key_search_device launch over the 128
flipped keys prepared on the host, on the same resident tuples: windows of `reps` launches
between device events, the two alternating, every window's time per launch reported."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rss_simulator_nvidia_amd import _native, keysearch  # noqa: E402

nbr = len(sys.argv) > 1 and sys.argv[1] == "neighbourhood"
K = 128 if nbr else int(sys.argv[1]) if len(sys.argv) > 1 else 1024
n = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 20
dist = sys.argv[3] if len(sys.argv) > 3 else "uniform"
H = int(sys.argv[4]) if len(sys.argv) > 4 else 128
Q = int(sys.argv[5]) if len(sys.argv) > 5 else 24
dev = torch.device("cuda:0")
s = torch.cuda.current_stream(dev).cuda_stream
base_key = keysearch.random_keys(1, seed=7)[0]
keys = ([keysearch.flip_bit(base_key, j) for j in range(K)] if nbr
        else keysearch.random_keys(K, seed=0))
win = np.stack([np.ctypeslib.as_array(_native.prepare_key(k).window) for k in keys])
windows = torch.from_numpy(win.astype(np.uint32).view(np.int32)).to(dev)
tuples = torch.empty(3 * n, dtype=torch.int32, device=dev)
counts = torch.empty((K, Q), dtype=torch.int64, device=dev)
if dist == "flow":
    import bench  # noqa: E402
    bench.flow_device(torch, tuples, 0, n, dev)
else:
    _native.generate_device(1, 0, n, tuples.data_ptr(), s)
run = lambda: _native.key_search_device(windows.data_ptr(), K, tuples.data_ptr(), n, H, Q,  # noqa
                                        counts.data_ptr(), s)


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


if nbr:
    prepared = _native.prepare_key(base_key)
    ncounts = torch.empty((K, Q), dtype=torch.int64, device=dev)
    new = lambda: _native.key_neighbourhood_device(prepared, tuples.data_ptr(), n, H, Q,  # noqa
                                                   ncounts.data_ptr(), s)
    for _ in range(20):  # warm both
        run()
        new()
    torch.cuda.synchronize()
    assert torch.equal(counts, ncounts) and int(ncounts.sum()) == K * n
    reps, rounds = 200, 7
    t_new, t_old = [], []
    for _ in range(rounds):
        t_old.append(window_ms(run, reps))
        t_new.append(window_ms(new, reps))
    med = lambda v: float(np.median(v))  # noqa: E731
    print(json.dumps({"mode": "neighbourhood", "distribution": dist, "flows": n, "htable": H,
                      "queues": Q, "reps_per_window": reps,
                      "search_128_keys_ms": t_old, "neighbourhood_ms": t_new,
                      "search_median_ms": med(t_old), "neighbourhood_median_ms": med(t_new),
                      "speedup": med(t_old) / med(t_new),
                      "key_tuple_evals_per_s": K * n / (med(t_new) / 1e3)}))
    sys.exit(0)

run()
torch.cuda.synchronize()
ms = window_ms(run, 5)
assert int(counts.sum()) == K * n
print(json.dumps({"distribution": dist, "keys": K, "flows": n, "htable": H, "queues": Q, "ms": ms,
                  "key_tuple_evals_per_s": K * n / (ms / 1e3),
                  "keys_per_s": K / (ms / 1e3)}))
