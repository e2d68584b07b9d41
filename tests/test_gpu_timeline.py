"""GPU parity for key search over time: rss_key_search_timeline_* against exact per-window,
per-queue sums of the weights over the oracle's queues -- tiles that end mid-group, slots in
and out of time order and past nslots, weights that wrap a 32-bit bin after two packets, each
side of every tier of the launcher's table; misaligned device input, graph replay, the CLI."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

TILE = 1024  # the smallest tile: one packet per lane


@pytest.fixture(scope="module")
def native():
    from rss_simulator_nvidia_amd import _native
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a gfx950 device")
    return _native


def loads_of(oracle_lib, keys, tuples, weights, slots, nslots, H, Q):
    """Exact uint64 loads [len(keys), nslots, min(H, Q)]: the weights summed per (slot, queue)."""
    ref = np.zeros((len(keys), nslots, min(H, Q)), dtype=np.uint64)
    ok = slots < nslots
    for k, key in enumerate(keys):
        if len(tuples):
            queues = oracle_lib.run(key, tuples, H, Q)[1]
            np.add.at(ref[k], (slots[ok], queues[ok]), weights[ok].astype(np.uint64))
    return ref


def make_weights(kind, n, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return np.full(n, 0xFFFFFFFF if kind == "max" else 1, dtype=np.uint32)  # "ones", None


def make_slots(pattern, n):
    """(slots, nslots) of n packets."""
    i = np.arange(n, dtype=np.int64)
    if pattern == "runs":  # non-decreasing, runs shorter and longer than a tile
        runs = np.tile([300, 2 * TILE + 452, 100, TILE + 476], n // 4000 + 1)
        s = np.repeat(np.arange(len(runs)), runs)[:n]
    elif pattern == "one":  # every packet in the last of four slots
        return np.full(n, 3, dtype=np.uint32), 4
    elif pattern == "single":  # nslots = 1
        return np.zeros(n, dtype=np.uint32), 1
    elif pattern == "span":  # ordered, a tile spans ~10 slots: more than any cache below holds
        s = i // 100
    elif pattern == "reversed":
        s = (n - 1 - i) // 100
    elif pattern == "mod":  # a jump on every packet
        s = i % 7
    else:  # "beyond": the later half of the windows, and every 50th packet, are >= nslots
        s = np.where(i % 50 == 49, 0xFFFFFFFF, i // 100)
        return s.astype(np.uint32), max(1, n // 200)
    return s.astype(np.uint32), int(s.max()) + 1 if n else 1


# 256 CUs and every slot cached: a tile of 9 x 1024 packets, 2304 groups for 1024 lanes
LOOPS = (1 << 21) + 5

CASES = [
    # tile lengths (H = 128, Q = 24: 8 keys per workgroup, 3 slots cached), patterns, weights
    (128, 24, 0, 11, "runs", "random"), (128, 24, 5, 11, "one", "max"),
    (128, 24, TILE + 3, 11, "runs", "random"), (128, 24, 5 * TILE - 117, 11, "runs", None),
    (128, 24, 5 * TILE - 117, 11, "runs", "ones"), (128, 24, 5 * TILE - 117, 11, "span", "random"),
    (128, 24, 5 * TILE - 117, 11, "reversed", "random"), (128, 24, 5 * TILE - 117, 11, "mod", "max"),
    (128, 24, 5 * TILE - 117, 11, "beyond", "random"), (128, 24, 5 * TILE - 117, 11, "single", "max"),
    (128, 24, 5 * TILE - 117, 3, "span", "random"), (128, 24, LOOPS, 2, "one", "random"),
    # packed tables: 8 keys to q = 38, 4 to 77, 2 to 154, shared bins to 2476 ...
    (256, 38, 2003, 11, "span", "random"), (256, 39, 2003, 11, "span", "random"),
    (1024, 77, 2003, 11, "span", "random"), (1024, 78, 2003, 11, "span", "random"),
    (1024, 154, 2003, 11, "span", "random"), (1024, 155, 2003, 11, "span", "random"),
    (4096, 2476, 2003, 11, "span", "max"), (4096, 2477, 2003, 11, "span", "random"),
    # ... pair tables: lane-private bins to q = 40, shared to 1280, then global atomics only
    (1000, 40, 2003, 11, "span", "random"), (1000, 41, 2003, 11, "span", "random"),
    (3000, 1280, 2003, 11, "span", "max"), (3000, 1281, 2003, 11, "beyond", "random"),
    (131072, 24, 2003, 11, "runs", "random"), (100000, 45000, 999, 3, "mod", "max"),
    (100, 7, 4097, 11, "runs", "ones"), (1, 1, 5, 3, "one", "max"), (16, 24, 2003, 11, "span", "random")]


@pytest.mark.parametrize("H,Q,n,nkeys,pattern,kind", CASES)
def test_timeline_loads_match_reference(native, oracle_lib, H, Q, n, nkeys, pattern, kind):
    from rss_simulator_nvidia_amd import keysearch
    keys = keysearch.random_keys(nkeys, seed=H + Q)
    tuples = oracle_lib.generate(H * 7 + n, 0, n)
    slots, nslots = make_slots(pattern, n)
    weights = make_weights(kind, n, Q)
    given = None if kind is None else weights
    loads = keysearch.timeline(keys, tuples, slots, H, Q, nslots=nslots, weights=given)
    assert loads.shape == (nkeys, nslots, min(H, Q)) and loads.dtype == np.uint64
    np.testing.assert_array_equal(loads, loads_of(oracle_lib, keys, tuples, weights, slots, nslots,
                                                  H, Q))
    if pattern != "beyond":  # every packet is in some window: the windows add up to the total
        np.testing.assert_array_equal(loads.sum(axis=1, dtype=np.uint64),
                                      keysearch.evaluate(keys, tuples, H, Q, weights=weights))


def device_windows(native, keys, dev):
    win = np.stack([np.ctypeslib.as_array(native.prepare_key(k).window) for k in keys])
    return torch.from_numpy(win.astype(np.uint32).view(np.int32)).to(dev)


def test_device_api_misaligned_input_and_stale_output(native, oracle_lib):
    """Tuples, weights and slots all at a pointer = 4 mod 16 (the one-packet-per-lane body) and
    the loads pre-filled with garbage (the clearing kernel)."""
    from rss_simulator_nvidia_amd import keysearch
    dev = torch.device("cuda:0")
    n, H, Q = 5003, 128, 24
    host = oracle_lib.generate(777, 0, n)
    weights = make_weights("random", n, 3)
    slots, nslots = make_slots("runs", n)
    d_t = torch.empty(3 * n + 1, dtype=torch.int32, device=dev)
    d_w = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_s = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_t[1:] = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    d_w[1:] = torch.from_numpy(weights.view(np.int32)).to(dev)
    d_s[1:] = torch.from_numpy(slots.view(np.int32)).to(dev)
    assert all(t[1:].data_ptr() % 16 == 4 for t in (d_t, d_w, d_s)) and n % 4
    keys = keysearch.random_keys(5, seed=1)
    found = torch.full((len(keys), nslots, Q), -7, dtype=torch.int64, device=dev)
    native.key_search_timeline_device(
        device_windows(native, keys, dev).data_ptr(), len(keys), d_t[1:].data_ptr(),
        d_w[1:].data_ptr(), d_s[1:].data_ptr(), n, nslots, H, Q, found.data_ptr(),
        torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(found.cpu().numpy().view(np.uint64),
                                  loads_of(oracle_lib, keys, host, weights, slots, nslots, H, Q))


def test_graph_replay_follows_the_slots(native, oracle_lib):
    """The captured call clears its loads itself: each replay gives the loads of the slots then
    in the buffer, over whatever the loads held before."""
    from rss_simulator_nvidia_amd import keysearch
    dev = torch.device("cuda:0")
    n, H, Q, nslots = 4099, 128, 24, 41
    host = oracle_lib.generate(21, 0, n)
    weights = make_weights("random", n, 9)
    d_t = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    d_w = torch.from_numpy(weights.view(np.int32)).to(dev)
    d_s = torch.zeros(n, dtype=torch.int32, device=dev)
    loads = torch.empty((4, nslots, Q), dtype=torch.int64, device=dev)
    keys = keysearch.random_keys(4, seed=2)
    d_win = device_windows(native, keys, dev)
    call = lambda: native.key_search_timeline_device(  # noqa: E731
        d_win.data_ptr(), len(keys), d_t.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), n, nslots, H,
        Q, loads.data_ptr(), torch.cuda.current_stream().cuda_stream)
    call()  # eager first: code objects loaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for pattern in ("span", "reversed", "mod"):
        slots = make_slots(pattern, n)[0]
        d_s.copy_(torch.from_numpy(slots.view(np.int32)))
        loads.fill_(3)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(loads.cpu().numpy().view(np.uint64),
                                      loads_of(oracle_lib, keys, host, weights, slots, nslots, H, Q))


def test_cli_prints_each_listed_keys_peak(native, oracle_lib, tmp_path, capsys):
    from rss_simulator_nvidia_amd import keysearch
    n, H, Q, width = 3001, 128, 24, 250  # milliseconds
    t = oracle_lib.generate(5, 0, n)
    times = 100000 + np.sort(np.random.default_rng(4).integers(0, 3000, n))
    size = np.random.default_rng(6).integers(40, 1501, n)
    ip = lambda a: ".".join(str((int(a) >> s) & 255) for s in (24, 16, 8, 0))  # noqa: E731
    rows = ["%s,%s,%d,%d,%d,%d" % (ip(a), ip(b), p >> 16, p & 0xFFFF, when, sz)
            for (a, b, p), when, sz in zip(t, times, size)]
    csv = tmp_path / "packets.csv"
    csv.write_text("src_ip,dst_ip,src_port,dst_port,t,bytes\n" + "\n".join(rows) + "\n")
    keysearch.main(["--ips-file", str(csv), "--htable-size", str(H), "--num-queues", str(Q),
                    "--keys", "6", "--top", "2", "--time-column", "t", "--window", str(width),
                    "--weight-column", "bytes"])
    lines = re.findall(r"^(\S+)  peak (\S+) at window (\d+) of (\d+)$", capsys.readouterr().out,
                       flags=re.M)
    assert len(lines) == 2
    slots, nslots = keysearch.window_slots(times, width)
    for text, value, window, count in lines:
        key = [int(b, 16) for b in text.split(":")]
        ref = keysearch.peak(loads_of(oracle_lib, [key], t, size.astype(np.uint32), slots, nslots,
                                      H, Q), H, Q)
        assert (value, int(window), int(count)) == ("%.4f" % ref["peak"][0], ref["window"][0], nslots)
