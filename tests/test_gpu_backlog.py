"""GPU parity for key search by backlog: rss_key_search_backlog_* against a plain numpy form of
each queue's max-plus recurrence over the oracle's queues -- segments and rounds that end one
packet early or late, backlogs carried over several segments, idle gaps, empty queues, equal
ticks, the arithmetic's bounds, each side of every tier of the launcher's table; misaligned
device input and a short workspace, graph replay, the CLI."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEG = 256     # the shortest segment
ROUND = 204   # packets per segment per round at 8 keys x 24 queues (5 segments per workgroup)


@pytest.fixture(scope="module")
def native():
    from rss_simulator_nvidia_amd import _native
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a gfx950 device")
    return _native


def peaks_of(oracle_lib, keys, tuples, weights, ticks, drain, H, Q):
    """Exact uint64 peaks [len(keys), min(H, Q)]: per queue, with S the running load and a =
    drain * tick, the backlog after packet i is S_i - a_i + max over j <= i of (a_j - S_(j-1))."""
    ref = np.zeros((len(keys), min(H, Q)), dtype=np.uint64)
    w_all, a_all = weights.astype(np.int64), np.int64(drain) * ticks.astype(np.int64)
    for k, key in enumerate(keys):
        queues = oracle_lib.run(key, tuples, H, Q)[1] if len(tuples) else np.zeros(0, np.uint32)
        for q in np.unique(queues):
            idx = queues == q
            w, a = w_all[idx], a_all[idx]
            S = np.cumsum(w)
            ref[k, q] = (S + np.maximum.accumulate(a - (S - w)) - a).max()
    return ref


def make_weights(kind, n, seed):
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    if kind == "small":  # below the drain of the "step" cases
        return np.random.default_rng(seed).integers(0, 1000, n).astype(np.uint32)
    return np.full(n, 0xFFFFFFFF if kind == "max" else 1, dtype=np.uint32)  # "ones", None


def make_ticks(pattern, n):
    i = np.arange(n, dtype=np.int64)
    if pattern == "bursts":  # runs of equal ticks, shorter and longer than a segment
        runs = np.tile([3, 40, 1, SEG + 70, 7, 2 * SEG + 9, 5], n // 900 + 1)
        t = np.repeat(np.arange(len(runs)) * 3, runs)[:n]
    elif pattern == "equal":
        t = np.full(n, 77)
    elif pattern == "step":  # one apart
        t = 5 + i
    elif pattern == "gap":  # nothing arrives for longer than any segment lasts, twice
        t = i // 4 + 10**6 * (i >= 300) + 10**7 * (i >= 2 * SEG + 1)
    else:  # "wide": up to the last tick there is
        t = (i * (2**32 - 1)) // max(n - 1, 1)
    return t.astype(np.uint32)


CASES = [
    # segment and round lengths (H = 128, Q = 24, 11 keys: 8 per workgroup, 5 segments side by
    # side), patterns, weights, drains
    (128, 24, 0, 11, "bursts", "random", 5), (128, 24, 1, 11, "bursts", "max", 5),
    (128, 24, ROUND - 1, 11, "bursts", "random", 1 << 28), (128, 24, ROUND, 11, "bursts", "random", 1 << 28),
    (128, 24, ROUND + 1, 11, "bursts", "random", 1 << 28), (128, 24, SEG - 1, 11, "bursts", "random", 1 << 28),
    (128, 24, SEG, 11, "bursts", None, 1), (128, 24, SEG + 1, 11, "bursts", "ones", 1),
    (128, 24, 5 * SEG - 1, 11, "bursts", "random", 1 << 30), (128, 24, 5 * SEG + 1, 11, "bursts", "random", 1 << 30),
    (128, 24, 3001, 11, "bursts", "random", 1 << 29), (128, 24, 3001, 11, "gap", "random", 1 << 20),
    (128, 24, 3001, 11, "equal", "random", 12345), (128, 24, 3001, 11, "step", "small", 1000),
    (128, 24, 3001, 11, "wide", "max", 2**31 - 1), (128, 24, 3001, 11, "wide", "max", 1),
    (128, 24, 3001, 11, "bursts", "random", 0), (128, 24, 3001, 3, "bursts", "random", 1 << 29),
    (128, 24, 3001, 1, "bursts", "random", 1 << 29),
    # a queue without a packet in a middle segment: 120 queues, 256 packets
    (128, 120, 3 * SEG - 68, 11, "bursts", "random", 1 << 29),
    # 8 keys to q = 128, 4 keys to q = 255 (power-of-two H <= 65536), then one key: u8 ids to
    # 255, u16 to 1024, LDS states to 4096
    (256, 128, 2003, 11, "bursts", "random", 1 << 29), (256, 129, 2003, 11, "bursts", "random", 1 << 29),
    (512, 24, 2003, 11, "bursts", "random", 1 << 29), (1024, 255, 2003, 3, "bursts", "random", 1 << 29),
    (1024, 256, 2003, 3, "bursts", "max", 1 << 29), (1000, 255, 2003, 2, "gap", "random", 1 << 20),
    (1000, 256, 2003, 2, "bursts", "random", 1 << 29), (131072, 24, 2003, 3, "bursts", "random", 1 << 29),
    (4096, 1024, 2003, 3, "bursts", "random", 1 << 29), (4096, 1025, 2003, 3, "bursts", "random", 1 << 29),
    (4096, 5000, 2003, 3, "wide", "max", 2**31 - 1), (100000, 4096, 2003, 2, "equal", "random", 7),
    (1, 1, 777, 3, "bursts", "max", 1 << 30), (16, 24, 2003, 11, "bursts", "random", 1 << 29)]


@pytest.mark.parametrize("H,Q,n,nkeys,pattern,kind,drain", CASES)
def test_backlog_peaks_match_reference(native, oracle_lib, H, Q, n, nkeys, pattern, kind, drain):
    from rss_simulator_nvidia_amd import keysearch
    keys = keysearch.random_keys(nkeys, seed=H + Q)
    tuples = oracle_lib.generate(H * 7 + n, 0, n)
    ticks = make_ticks(pattern, n)
    weights = make_weights(kind, n, Q)
    given = None if kind is None else weights
    peaks = keysearch.backlog(keys, tuples, ticks, drain, H, Q, weights=given)
    assert peaks.shape == (nkeys, min(H, Q)) and peaks.dtype == np.uint64
    np.testing.assert_array_equal(peaks, peaks_of(oracle_lib, keys, tuples, weights, ticks, drain,
                                                  H, Q))
    if drain == 0 or pattern == "equal":  # nothing drains between arrivals: the load
        np.testing.assert_array_equal(peaks, keysearch.evaluate(keys, tuples, H, Q,
                                                                weights=weights))


def test_long_stream_matches_reference(native, oracle_lib):
    """Segments longer than one round of the workgroup, on a device of any size."""
    from rss_simulator_nvidia_amd import keysearch
    n, H, Q = (1 << 20) + 3, 128, 24
    keys = keysearch.random_keys(2, seed=8)
    tuples = oracle_lib.generate(99, 0, n)
    ticks = make_ticks("bursts", n)
    weights = make_weights("random", n, 5)
    np.testing.assert_array_equal(
        keysearch.backlog(keys, tuples, ticks, 1 << 30, H, Q, weights=weights),
        peaks_of(oracle_lib, keys, tuples, weights, ticks, 1 << 30, H, Q))


def device_windows(native, keys, dev):
    win = np.stack([np.ctypeslib.as_array(native.prepare_key(k).window) for k in keys])
    return torch.from_numpy(win.astype(np.uint32).view(np.int32)).to(dev)


def test_device_api_misaligned_input_stale_output_and_short_workspace(native, oracle_lib):
    """Tuples, weights and ticks all at a pointer = 4 mod 16, the peaks pre-filled with garbage,
    the workspace exactly the size the library asks for; one byte less is refused."""
    from rss_simulator_nvidia_amd import keysearch
    from rss_simulator_nvidia_amd.exceptions import DeviceError
    dev = torch.device("cuda:0")
    n, H, Q, drain = 5003, 128, 24, 1 << 29
    host = oracle_lib.generate(777, 0, n)
    weights = make_weights("random", n, 3)
    ticks = make_ticks("bursts", n)
    d_t = torch.empty(3 * n + 1, dtype=torch.int32, device=dev)
    d_w = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_s = torch.empty(n + 1, dtype=torch.int32, device=dev)
    d_t[1:] = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    d_w[1:] = torch.from_numpy(weights.view(np.int32)).to(dev)
    d_s[1:] = torch.from_numpy(ticks.view(np.int32)).to(dev)
    assert all(t[1:].data_ptr() % 16 == 4 for t in (d_t, d_w, d_s)) and n % 4
    keys = keysearch.random_keys(5, seed=1)
    need = native.key_search_backlog_workspace_bytes(len(keys), n, H, Q)
    ws = torch.full((need // 8,), -3, dtype=torch.int64, device=dev)
    found = torch.full((len(keys), Q), -7, dtype=torch.int64, device=dev)
    call = lambda size: native.key_search_backlog_device(  # noqa: E731
        device_windows(native, keys, dev).data_ptr(), len(keys), d_t[1:].data_ptr(),
        d_w[1:].data_ptr(), d_s[1:].data_ptr(), n, drain, H, Q, found.data_ptr(), ws.data_ptr(),
        size, torch.cuda.current_stream(dev).cuda_stream)
    with pytest.raises(DeviceError, match="workspace of %d bytes.* need %d" % (need - 1, need)):
        call(need - 1)
    call(need)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(found.cpu().numpy().view(np.uint64),
                                  peaks_of(oracle_lib, keys, host, weights, ticks, drain, H, Q))


def test_graph_replay_follows_the_ticks(native, oracle_lib):
    """The captured call writes every peak itself: each replay gives the peaks of the ticks then
    in the buffer, over whatever the peaks and the workspace held before."""
    from rss_simulator_nvidia_amd import keysearch
    dev = torch.device("cuda:0")
    n, H, Q, drain = 4099, 128, 24, 1 << 20
    host = oracle_lib.generate(21, 0, n)
    weights = make_weights("random", n, 9)
    d_t = torch.from_numpy(host.view(np.int32).reshape(-1)).to(dev)
    d_w = torch.from_numpy(weights.view(np.int32)).to(dev)
    d_s = torch.zeros(n, dtype=torch.int32, device=dev)
    peaks = torch.empty((4, Q), dtype=torch.int64, device=dev)
    keys = keysearch.random_keys(4, seed=2)
    d_win = device_windows(native, keys, dev)
    need = native.key_search_backlog_workspace_bytes(len(keys), n, H, Q)
    ws = torch.empty(need // 8, dtype=torch.int64, device=dev)
    call = lambda: native.key_search_backlog_device(  # noqa: E731
        d_win.data_ptr(), len(keys), d_t.data_ptr(), d_w.data_ptr(), d_s.data_ptr(), n, drain, H,
        Q, peaks.data_ptr(), ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream)
    call()  # eager first: code objects loaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for pattern in ("bursts", "gap", "step"):
        ticks = make_ticks(pattern, n)
        d_s.copy_(torch.from_numpy(ticks.view(np.int32)))
        peaks.fill_(3)
        ws.fill_(-1)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(peaks.cpu().numpy().view(np.uint64),
                                      peaks_of(oracle_lib, keys, host, weights, ticks, drain, H, Q))


def test_cli_prints_each_listed_keys_backlog(native, oracle_lib, tmp_path, capsys):
    from rss_simulator_nvidia_amd import keysearch
    n, H, Q, width, drain = 3001, 128, 24, 2.5, 700  # milliseconds; bytes per tick
    t = oracle_lib.generate(5, 0, n)
    times = 100000 + np.random.default_rng(4).integers(0, 3000, n)  # not in time order
    size = np.random.default_rng(6).integers(40, 1501, n)
    ip = lambda a: ".".join(str((int(a) >> s) & 255) for s in (24, 16, 8, 0))  # noqa: E731
    rows = ["%s,%s,%d,%d,%d,%d" % (ip(a), ip(b), p >> 16, p & 0xFFFF, when, sz)
            for (a, b, p), when, sz in zip(t, times, size)]
    csv = tmp_path / "packets.csv"
    csv.write_text("src_ip,dst_ip,src_port,dst_port,t,bytes\n" + "\n".join(rows) + "\n")
    keysearch.main(["--ips-file", str(csv), "--htable-size", str(H), "--num-queues", str(Q),
                    "--keys", "6", "--top", "2", "--time-column", "t", "--window", "250",
                    "--weight-column", "bytes", "--drain", str(drain), "--tick", str(width)])
    out = capsys.readouterr().out
    lines = re.findall(r"^(\S+)  backlog (\d+) at queue (\d+)$", out, flags=re.M)
    assert len(lines) == 2 and len(re.findall(r"  peak ", out)) == 2
    ticks = keysearch.window_slots(times, width)[0]
    order = np.argsort(ticks, kind="stable")
    for text, value, queue in lines:
        key = [int(b, 16) for b in text.split(":")]
        ref = peaks_of(oracle_lib, [key], t[order], size[order].astype(np.uint32), ticks[order],
                       drain, H, Q)[0]
        assert (int(value), int(queue)) == (ref.max(), ref.argmax())
