"""Flow-aggregation throughput (tool, not product): packets to flows on the device.
usage: python tools/aggregate_bench.py device [--out DIR] [log2_n ...]      (default 24 26)
       python tools/aggregate_bench.py host [--out DIR] [log2_n ...]        (default 22 24)
device times rss_flow_aggregate_device on resident packets with u32 weights, IPv4 and IPv6, on
two inputs -- Zipf(1.2) draws from 2^20 flows and all-distinct tuples -- with the LDS combiner
on and off (RSS_AGGREGATE_COMBINER=0) in alternating windows between device events, medians.
Each row gives packets/s and the share of the pipeline's byte floor at HBM_BYTES_PER_S:
    clear      12 B per table slot (cap = the power of two >= 2n)
    input      4 (words + 1) B per packet
    slot_of    4 B per packet, written once and read twice
    output     (4 words + 12) B per flow
host times rss_flow_aggregate_host (upload, pipeline, download of the F rows) against the
np.unique block of pcap.read_flows on the same IPv4 arrays on this machine's CPU, and checks
that both give the same flows and loads.
Writes DIR/device.json or DIR/host.json (default profiles/aggregate)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from rss_simulator_nvidia_amd import _native  # noqa: E402

HBM_BYTES_PER_S = 8.0e12  # MI355X HBM3E peak
ZIPF_FLOWS = 1 << 20
DEV = torch.device("cuda:0")


def window_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def random_words(rows, words, seed):
    g = torch.Generator(DEV).manual_seed(seed)
    return torch.randint(0, 2**32, (rows, words), dtype=torch.int64, device=DEV,
                         generator=g).to(torch.int32)


def make_packets(kind, n, words, seed=1):
    """(n, words) int32 packets on the device: Zipf(1.2) ranks into a flow table, or distinct."""
    if kind == "distinct":
        t = random_words(n, words, seed)
        # an odd multiplier is a bijection of the 32-bit indices: no two rows equal
        t[:, 0] = (torch.arange(n, dtype=torch.int64, device=DEV) * 0x9E3779B1).to(torch.int32)
        return t
    cdf = torch.cumsum(torch.arange(1, ZIPF_FLOWS + 1, dtype=torch.float64, device=DEV) ** -1.2, 0)
    u = torch.rand(n, dtype=torch.float64, device=DEV,
                   generator=torch.Generator(DEV).manual_seed(seed)) * cdf[-1]
    ranks = torch.searchsorted(cdf, u).clamp_(max=ZIPF_FLOWS - 1)
    table = random_words(ZIPF_FLOWS, words, seed + 1)
    table[:, 0] = (torch.arange(ZIPF_FLOWS, dtype=torch.int64, device=DEV) * 0x9E3779B1).to(torch.int32)
    return table[ranks].contiguous()


def floor_bytes(n, words, nflows):
    cap = max(1024, 1 << (2 * n - 1).bit_length())
    return 12 * cap + 4 * (words + 1) * n + 3 * 4 * n + (4 * words + 12) * nflows


def device_main(out_dir, logs, reps=5, rounds=5):
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rows = []
    for log_n in logs:
        n = 1 << log_n
        for words in (3, 9):
            for kind in ("zipf", "distinct"):
                packets = make_packets(kind, n, words)
                weights = torch.randint(40, 1501, (n,), dtype=torch.int32, device=DEV,
                                        generator=torch.Generator(DEV).manual_seed(3))
                ws_bytes = _native.flow_aggregate_workspace_bytes(n, words)
                ws = torch.empty(ws_bytes // 8, dtype=torch.int64, device=DEV)
                flows = torch.empty((n, words), dtype=torch.int32, device=DEV)
                loads = torch.empty(n, dtype=torch.int64, device=DEV)
                first = torch.empty(n, dtype=torch.int32, device=DEV)
                nflows = torch.zeros(1, dtype=torch.int64, device=DEV)

                def call():
                    _native.flow_aggregate_device(
                        packets.data_ptr(), words, weights.data_ptr(), n, flows.data_ptr(),
                        loads.data_ptr(), first.data_ptr(), nflows.data_ptr(), ws.data_ptr(),
                        ws_bytes, stream)

                times, found = {"1": [], "0": []}, {}
                for combiner in ("1", "0"):  # warm both, and check they agree
                    os.environ["RSS_AGGREGATE_COMBINER"] = combiner
                    call()
                    torch.cuda.synchronize()
                    f = int(nflows.cpu()[0])
                    found[combiner] = (f, int(loads[:f].sum().cpu()), int(first[:f].sum().cpu()))
                assert found["1"] == found["0"] and found["1"][1] == int(weights.sum().cpu()), found
                for _ in range(rounds):
                    for combiner in ("1", "0"):
                        os.environ["RSS_AGGREGATE_COMBINER"] = combiner
                        times[combiner].append(window_ms(call, reps))
                os.environ.pop("RSS_AGGREGATE_COMBINER")
                f = found["1"][0]
                floor = floor_bytes(n, words, f)
                row = {"n": n, "words": words, "input": kind, "flows": f, "floor_bytes": floor}
                for combiner, name in (("1", "combiner"), ("0", "direct")):
                    ms = float(np.median(times[combiner]))
                    row[name] = {"ms": ms, "windows_ms": times[combiner],
                                 "packets_per_s": n / (ms * 1e-3),
                                 "share_of_byte_floor": floor / HBM_BYTES_PER_S / (ms * 1e-3)}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del packets, weights, ws, flows, loads, first
                torch.cuda.empty_cache()
    save(out_dir, "device", {"hbm_bytes_per_s": HBM_BYTES_PER_S, "reps": reps, "rounds": rounds,
                             "rows": rows})


def numpy_unique(tuples):
    """The np.unique block of pcap.read_flows."""
    raw = np.ascontiguousarray(tuples).view(np.dtype((np.void, tuples.dtype.itemsize)))
    _, first, per_flow = np.unique(raw, return_index=True, return_counts=True)
    by_first = np.argsort(first, kind="stable")
    order = first[by_first]
    return tuples[order], per_flow[by_first].astype(np.uint32)


def host_main(out_dir, logs):
    ctx = _native.default_context()
    rows = []
    for log_n in logs:
        n = 1 << log_n
        for kind in ("zipf", "distinct"):
            tuples = make_packets(kind, n, 3).cpu().numpy().view(_native.TUPLE_DTYPE).reshape(-1)
            ctx.aggregate_flows(tuples[:4096])  # code objects loaded
            device_s = []
            for _ in range(3):
                t0 = time.perf_counter()
                flows, loads, _ = ctx.aggregate_flows(tuples)
                device_s.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            want_flows, want_counts = numpy_unique(tuples)
            numpy_s = time.perf_counter() - t0
            assert np.array_equal(flows.view(_native.TUPLE_DTYPE).reshape(-1), want_flows)
            assert np.array_equal(loads, want_counts)
            d = float(np.median(device_s))
            row = {"n": n, "input": kind, "flows": len(flows), "host_entry_s": d,
                   "host_entry_runs_s": device_s, "numpy_unique_s": numpy_s,
                   "host_entry_packets_per_s": n / d, "numpy_packets_per_s": n / numpy_s,
                   "speedup": numpy_s / d}
            print(json.dumps(row), flush=True)
            rows.append(row)
    save(out_dir, "host", {"cpus": os.cpu_count(), "rows": rows})


def save(out_dir, name, result):
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, name + ".json"), "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "aggregate")
    if "--out" in argv:
        at = argv.index("--out")
        out = argv[at + 1]
        del argv[at:at + 2]
    mode, logs = argv[0], [int(a) for a in argv[1:]]
    if mode == "device":
        device_main(out, logs or [24, 26])
    else:
        host_main(out, logs or [22, 24])
