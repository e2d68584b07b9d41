"""Key-search throughput (tool, not product): K random keys x n resident flows, one launch.
Prints key-tuple evaluations per second.
usage: python tools/keysearch_bench.py [K] [n] [uniform|flow] [H] [Q]
       python tools/keysearch_bench.py neighbourhood [n] [uniform|flow] [H] [Q]
The neighbourhood mode times one rss_key_neighbourhood_device launch (the 128 single-bit
flips of one key) against the same job as one rss_key_search_device launch over the 128
flipped keys prepared on the host, on the same resident tuples: windows of `reps` launches
between device events, the two alternating, every window's time per launch reported.
       python tools/keysearch_bench.py --ipv6 [K] [n] [H] [Q]
       python tools/keysearch_bench.py --ipv6 neighbourhood [n] [H] [Q]
--ipv6 times the IPv6 entries on n resident uniform 36-byte tuples: one rss_key_search6_device
launch over K keys against K back-to-back counts-only rss_hash6_device launches (all there was
before it), and one rss_key_neighbourhood6_device launch against one rss_key_search6_device
launch over the 320 host-prepared flipped keys and against 320 rss_hash6_device launches; the
contenders alternate, `rounds` windows each, medians reported.
       python tools/keysearch_bench.py --weighted [n] [H] [Q] [K]
--weighted times key search by load on n resident uniform tuples: rss_key_search_weighted_device
over K keys and rss_key_neighbourhood_weighted_device, each with heavy-tailed weights (Zipf 1.3,
clipped to u32) and with all-ones weights, against the unweighted entries at the same shape in
the same process (alternating windows, medians), and against the host loop they replace: one
rss_hash_device launch per key, its queue column copied back and np.bincount(weights=) on the
host, timed over 16 keys and scaled to K.  One shape per invocation, so that a job gives each
shape a time limit of its own.
       python tools/keysearch_bench.py --symmetric [n] [H] [Q] [big_n]
--symmetric times the exhaustive symmetric-key ranking on n resident uniform flows: the fold
alone (rss_symmetric_fold_device: IPv4, IPv6, IPv4 with weights), the scan of all 65536 patterns
alone (rss_symmetric_search_device) and the two together, against the only way there was before:
one rss_key_search_device launch over the 65536 periodic keys' windows (built once, outside the
timing; its counts compared equal to the new loads first).  Alternating windows between device
events, medians.  Then the fold at big_n flows against the tuple bytes it has to read."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rss_simulator_nvidia_amd import _native, keysearch  # noqa: E402


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def ipv6_main(argv):
    """--ipv6 [neighbourhood] ...: see the module docstring."""
    nbr = bool(argv) and argv[0] == "neighbourhood"
    num = [int(a) for a in argv[1 if nbr else 0:]]
    K = 320 if nbr else (num.pop(0) if num else 1024)
    n, H, Q = (num + [1 << 20, 128, 24][len(num):])[:3]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    base_key = keysearch.random_keys(1, seed=7)[0]
    keys = ([keysearch.flip_bit(base_key, j) for j in range(K)] if nbr
            else keysearch.random_keys(K, seed=0))
    prepared = [_native.prepare_key6(k) for k in keys]
    win = np.stack([np.ctypeslib.as_array(k.window) for k in prepared]).astype(np.uint32)
    windows = torch.from_numpy(win.view(np.int32)).to(dev)
    tuples = torch.randint(0, 2**32, (9 * n,), dtype=torch.int64, device=dev,
                           generator=torch.Generator(dev).manual_seed(1)).to(torch.int32)
    width = _native.queue_modulus(H, Q)[1]
    c_search = torch.empty((K, width), dtype=torch.int64, device=dev)
    c_loop = torch.empty((K, width), dtype=torch.int64, device=dev)
    search = lambda: _native.key_search6_device(windows.data_ptr(), K, tuples.data_ptr(), n, H, Q,  # noqa
                                                c_search.data_ptr(), s)

    def loop():  # one counts-only hash launch per key
        for k in range(K):
            _native.hash6_device(prepared[k], tuples.data_ptr(), n, H, Q, None, None,
                                 c_loop[k].data_ptr(), 0, s)

    contenders = {"search6": (search, 50), "hash6_loop": (loop, 3)}
    if nbr:
        c_nbr = torch.empty((K, width), dtype=torch.int64, device=dev)
        base = _native.prepare_key6(base_key)
        contenders["neighbourhood6"] = (
            lambda: _native.key_neighbourhood6_device(base, tuples.data_ptr(), n, H, Q,
                                                      c_nbr.data_ptr(), s), 50)
    for fn, _ in contenders.values():  # warm, then check every contender against the loop
        fn()
        fn()
    torch.cuda.synchronize()
    assert torch.equal(c_search, c_loop) and int(c_loop.sum()) == K * n
    assert not nbr or torch.equal(c_nbr, c_loop)
    rounds = 7
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, (fn, reps) in contenders.items():
            times[name].append(window_ms(fn, reps))
    med = {name: float(np.median(v)) for name, v in times.items()}
    best = med["neighbourhood6" if nbr else "search6"]
    out = {"mode": "ipv6 " + ("neighbourhood" if nbr else "search"), "keys": K, "flows": n,
           "htable": H, "queues": Q, "window_ms": times, "median_ms": med,
           "key_flow_evals_per_s": K * n / (best / 1e3),
           "speedup_vs_hash6_loop": med["hash6_loop"] / best}
    if nbr:
        out["speedup_vs_search6"] = med["search6"] / best
    print(json.dumps(out))


def weighted_main(argv):
    """--weighted [n] [H] [Q] [K]: see the module docstring."""
    import time
    n, H, Q, K = ([int(a) for a in argv] + [1 << 20, 128, 24, 1024][len(argv):])[:4]
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    base_key = keysearch.random_keys(1, seed=7)[0]
    base = _native.prepare_key(base_key)
    prepared = [_native.prepare_key(k) for k in keysearch.random_keys(K, seed=0)]
    win = np.stack([np.ctypeslib.as_array(k.window) for k in prepared]).astype(np.uint32)
    windows = torch.from_numpy(win.view(np.int32)).to(dev)
    tuples = torch.empty(3 * n, dtype=torch.int32, device=dev)
    _native.generate_device(1, 0, n, tuples.data_ptr(), s)
    rng = np.random.default_rng(3)
    host_w = {"zipf": np.minimum(rng.zipf(1.3, n), 0xFFFFFFFF).astype(np.uint32),
              "ones": np.ones(n, dtype=np.uint32)}
    d_w = {name: torch.from_numpy(w.view(np.int32)).to(dev) for name, w in host_w.items()}
    width = _native.queue_modulus(H, Q)[1]
    out = {name: torch.empty((rows, width), dtype=torch.int64, device=dev)
           for name, rows in (("search", K), ("search_zipf", K), ("search_ones", K),
                              ("neighbourhood", 128), ("neighbourhood_zipf", 128),
                              ("neighbourhood_ones", 128))}
    contenders = {
        "search": (lambda: _native.key_search_device(
            windows.data_ptr(), K, tuples.data_ptr(), n, H, Q, out["search"].data_ptr(), s), 100),
        "neighbourhood": (lambda: _native.key_neighbourhood_device(
            base, tuples.data_ptr(), n, H, Q, out["neighbourhood"].data_ptr(), s), 500)}
    for name in host_w:
        contenders["search_" + name] = (lambda name=name: _native.key_search_weighted_device(
            windows.data_ptr(), K, tuples.data_ptr(), d_w[name].data_ptr(), n, H, Q,
            out["search_" + name].data_ptr(), s), 100)
        contenders["neighbourhood_" + name] = (
            lambda name=name: _native.key_neighbourhood_weighted_device(
                base, tuples.data_ptr(), d_w[name].data_ptr(), n, H, Q,
                out["neighbourhood_" + name].data_ptr(), s), 500)
    for fn, _ in contenders.values():  # warm every shape, then check before timing
        for _ in range(10):
            fn()
    torch.cuda.synchronize()
    total = int(host_w["zipf"].sum(dtype=np.uint64))
    for kind in ("search", "neighbourhood"):
        assert torch.equal(out[kind + "_ones"], out[kind])
        assert bool((out[kind + "_zipf"].sum(dim=1) == total).all())

    # the host loop the weighted search replaces, over 16 keys
    queues = torch.empty(n, dtype=torch.int32, device=dev)
    loop_keys = 16
    weights64 = host_w["zipf"].astype(np.float64)  # sums < 2^53: exact
    loop_loads = np.zeros((loop_keys, width))

    def host_loop():
        for k in range(loop_keys):
            _native.hash_device(prepared[k], tuples.data_ptr(), n, H, Q, None, queues.data_ptr(),
                                None, 0, s)
            loop_loads[k] = np.bincount(queues.cpu().numpy(), weights=weights64, minlength=width)

    host_loop()  # warm
    assert np.array_equal(loop_loads.astype(np.uint64),
                          out["search_zipf"][:loop_keys].cpu().numpy().view(np.uint64))
    loop_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        host_loop()
        loop_ms.append((time.perf_counter() - t0) * 1e3 * K / loop_keys)

    rounds = 7
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, (fn, reps) in contenders.items():
            times[name].append(window_ms(fn, reps))
    med = {name: float(np.median(v)) for name, v in times.items()}
    print(json.dumps({
        "mode": "weighted", "keys": K, "flows": n, "htable": H, "queues": Q,
        "reps_per_window": {name: reps for name, (_, reps) in contenders.items()},
        "window_ms": times, "median_ms": med,
        "host_loop_ms_scaled_to_keys": loop_ms, "host_loop_keys_timed": loop_keys,
        "host_loop_median_ms": float(np.median(loop_ms)),
        "search_weighted_over_unweighted": {k: med["search_" + k] / med["search"] for k in host_w},
        "neighbourhood_weighted_over_unweighted": {
            k: med["neighbourhood_" + k] / med["neighbourhood"] for k in host_w},
        "host_loop_over_search_weighted": float(np.median(loop_ms)) / med["search_zipf"],
        "search_weighted_key_flow_evals_per_s": K * n / (med["search_zipf"] / 1e3),
        "neighbourhood_weighted_key_flow_evals_per_s": 128 * n / (med["neighbourhood_zipf"] / 1e3)}))


def symmetric_main(argv):
    """--symmetric [n] [H] [Q] [big_n]: see the module docstring."""
    n, H, Q, big_n = ([int(a) for a in argv] + [1 << 20, 128, 24, 1 << 26][len(argv):])[:4]
    P = _native.SYMMETRIC_PATTERNS
    dev = torch.device("cuda:0")
    s = torch.cuda.current_stream(dev).cuda_stream
    t4 = torch.empty(3 * n, dtype=torch.int32, device=dev)
    _native.generate_device(1, 0, n, t4.data_ptr(), s)
    t6 = torch.randint(0, 2**32, (9 * n,), dtype=torch.int64, device=dev,
                       generator=torch.Generator(dev).manual_seed(1)).to(torch.int32)
    host_w = np.minimum(np.random.default_rng(3).zipf(1.3, n), 0xFFFFFFFF).astype(np.uint32)
    d_w = torch.from_numpy(host_w.view(np.int32)).to(dev)
    width = _native.queue_modulus(H, Q)[1]
    folds = {k: torch.empty(P, dtype=torch.int64, device=dev) for k in ("v4", "v6", "v4w")}
    loads = torch.empty((P, width), dtype=torch.int64, device=dev)
    # the periodic keys' windows in closed form: window i = rotl16(p, i % 16) twice over
    p = np.arange(P, dtype=np.uint32)[:, None]
    r = (np.arange(96, dtype=np.uint32) % 16)[None, :]
    g = ((p << r) | (p >> (16 - r))) & 0xFFFF
    win = (g << 16) | g
    for pat in (0, 1, 0x6d5a, 0xFFFF):
        key = _native.prepare_key(keysearch.symmetric_key(pat))
        assert np.array_equal(win[pat], np.ctypeslib.as_array(key.window))
    windows = torch.from_numpy(win.view(np.int32)).to(dev)
    counts = torch.empty((P, width), dtype=torch.int64, device=dev)

    def fold(kind):
        tuples, words, w = {"v4": (t4, 3, None), "v6": (t6, 9, None), "v4w": (t4, 3, d_w)}[kind]
        return lambda: _native.symmetric_fold_device(
            tuples.data_ptr(), words, _native.FIELDS_ALL, w.data_ptr() if w is not None else None,
            n, folds[kind].data_ptr(), 0, s)

    scan = lambda: _native.symmetric_search_device(folds["v4"].data_ptr(), 0, P, H, Q,  # noqa: E731
                                                   loads.data_ptr(), s)
    contenders = {
        "fold_ipv4": (fold("v4"), 200), "fold_ipv6": (fold("v6"), 200),
        "fold_ipv4_weighted": (fold("v4w"), 200), "scan": (scan, 20),
        "fold_and_scan": (lambda: (fold("v4")(), scan()), 20),
        "search_65536_keys": (lambda: _native.key_search_device(
            windows.data_ptr(), P, t4.data_ptr(), n, H, Q, counts.data_ptr(), s), 2)}
    for fn, _ in contenders.values():  # warm every shape, then check before timing
        fn()
        fn()
    torch.cuda.synchronize()
    assert torch.equal(loads, counts) and bool((loads.sum(dim=1) == n).all())
    assert int(folds["v6"].sum()) == n and int(folds["v4w"].sum()) == int(host_w.sum(dtype=np.uint64))
    rounds = 5
    times = {name: [] for name in contenders}
    for _ in range(rounds):
        for name, (fn, reps) in contenders.items():
            times[name].append(window_ms(fn, reps))
    med = {name: float(np.median(v)) for name, v in times.items()}
    # the fold at big_n flows: the tuples are the bytes it has to read (each quarter reads them)
    del t6, windows, counts
    big = torch.empty(3 * big_n, dtype=torch.int32, device=dev)
    _native.generate_device(2, 0, big_n, big.data_ptr(), s)
    big_fold = lambda: _native.symmetric_fold_device(big.data_ptr(), 3, _native.FIELDS_ALL, None,  # noqa
                                                     big_n, folds["v4"].data_ptr(), 0, s)
    big_fold()
    torch.cuda.synchronize()
    assert int(folds["v4"].sum()) == big_n
    big_ms = [window_ms(big_fold, 10) for _ in range(rounds)]
    print(json.dumps({
        "mode": "symmetric", "flows": n, "htable": H, "queues": Q, "patterns": P,
        "reps_per_window": {name: reps for name, (_, reps) in contenders.items()},
        "window_ms": times, "median_ms": med,
        "scan_fold_pattern_evals_per_s": P * P / (med["scan"] / 1e3),
        "search_key_flow_evals_per_s": P * n / (med["search_65536_keys"] / 1e3),
        "speedup_vs_search_65536_keys": med["search_65536_keys"] / med["fold_and_scan"],
        "big_fold": {"flows": big_n, "window_ms": big_ms, "median_ms": float(np.median(big_ms)),
                     "tuple_bytes": 12 * big_n,
                     "tuple_gb_per_s": 12 * big_n / (float(np.median(big_ms)) / 1e3) / 1e9}}))


if len(sys.argv) > 1 and sys.argv[1] == "--symmetric":
    symmetric_main(sys.argv[2:])
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--weighted":
    weighted_main(sys.argv[2:])
    sys.exit(0)

if len(sys.argv) > 1 and sys.argv[1] == "--ipv6":
    ipv6_main(sys.argv[2:])
    sys.exit(0)

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
