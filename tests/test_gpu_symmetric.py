"""GPU parity for symmetric RSS: rss_symmetric_fold_device against a numpy fold, the pattern
scan against the oracle run on the literal 40-byte symmetric keys (every bin tier of the
launcher, IPv4 and IPv6, weights, a field selection), the whole range's invariants, graph
replay, and the --symmetric CLI on a CSV and an IPv6 capture."""
import re

import numpy as np
import pytest

import pcap_builder as pb

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PATTERNS = [(0, 1), (1, 1), (0x8000, 1), (0x6d5a, 1), (0xFFFF, 1), (0x6d55, 11)]  # (first, count)


@pytest.fixture(scope="module")
def native():
    from rss_simulator_nvidia_amd import _native
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a gfx950 device")
    return _native


def random_words(n, words, seed):
    return np.random.default_rng(seed).integers(0, 2**32, (n, words), dtype=np.uint64).astype(np.uint32)


def make_weights(kind, n, seed):
    if kind == "none":
        return None
    if kind == "max":
        return np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    return random_words(n, 1, seed).reshape(-1)


def field_columns(words, fields):
    """The selected fields' words of (n, 3 | 9) tuples, ports masked by half: the oracle's
    hash input when the ports are whole or absent, and the fold's input always."""
    a = (words.shape[1] - 1) // 2
    keep = np.zeros(words.shape[1], dtype=np.uint32)
    keep[:a] = 0xFFFFFFFF if fields & 1 else 0
    keep[a:2 * a] = 0xFFFFFFFF if fields & 2 else 0
    keep[2 * a] = (0xFFFF0000 if fields & 4 else 0) | (0xFFFF if fields & 8 else 0)
    return words[:, keep != 0] & keep[keep != 0]


def fold_reference(words, fields, weights):
    x = np.bitwise_xor.reduce(field_columns(words, fields), axis=1) if len(words) else np.zeros(0, np.uint32)
    folds = np.zeros(65536, dtype=np.uint64)
    w = np.ones(len(words), np.uint64) if weights is None else weights.astype(np.uint64)
    np.add.at(folds, (x >> 16) ^ (x & 0xFFFF), w)
    return folds


def oracle_loads(oracle_lib, patterns, words, weights, H, Q, fields=15):
    """Exact loads of the literal symmetric keys: the weights summed per oracle queue."""
    from rss_simulator_nvidia_amd import keysearch
    w = np.ones(len(words), np.uint64) if weights is None else weights.astype(np.uint64)
    out = np.zeros((len(patterns), min(H, Q)), dtype=np.uint64)
    for row, p in zip(out, patterns):
        np.add.at(row, oracle_lib.run_words(keysearch.symmetric_key(p), field_columns(words, fields),
                                            H, Q)[1], w)
    return out


def to_device(array, offset_words=0):
    """`array` on the GPU behind `offset_words` int32 of padding (a pointer = 4 mod 16 for 1)."""
    flat = torch.from_numpy(np.ascontiguousarray(array).view(np.int32).reshape(-1))
    buf = torch.empty(len(flat) + offset_words, dtype=torch.int32, device="cuda:0")
    buf[offset_words:] = flat.to("cuda:0")
    return buf[offset_words:]


@pytest.mark.parametrize("fields", [15, 3, 12])
@pytest.mark.parametrize("n", [0, 5, 4099])
@pytest.mark.parametrize("kind", ["none", "random", "max"])
@pytest.mark.parametrize("words", [3, 9])
def test_fold_matches_numpy(native, words, kind, n, fields):
    tuples, weights = random_words(n, words, n + words), make_weights(kind, n, fields)
    d_t = to_device(tuples)
    d_w = to_device(weights) if weights is not None else None
    folds = torch.full((65536,), 7, dtype=torch.int64, device="cuda:0")
    native.symmetric_fold_device(d_t.data_ptr(), words, fields, d_w.data_ptr() if kind != "none"
                                 else None, n, folds.data_ptr())
    np.testing.assert_array_equal(folds.cpu().numpy().view(np.uint64),
                                  fold_reference(tuples, fields, weights))


@pytest.mark.parametrize("words", [3, 9])
def test_fold_misaligned_input_and_accumulate(native, words):
    """Tuples and weights at a pointer = 4 mod 16 over garbage folds; then two accumulating
    batches (the second aligned) equal one."""
    n = 4099
    tuples, weights = random_words(n, words, 3), make_weights("random", n, 4)
    d_t, d_w = to_device(tuples, 1), to_device(weights, 1)
    assert d_t.data_ptr() % 16 == 4 and d_w.data_ptr() % 16 == 4
    folds = torch.full((65536,), -3, dtype=torch.int64, device="cuda:0")
    native.symmetric_fold_device(d_t.data_ptr(), words, 15, d_w.data_ptr(), n, folds.data_ptr())
    want = fold_reference(tuples, 15, weights)
    np.testing.assert_array_equal(folds.cpu().numpy().view(np.uint64), want)
    half = 2048
    native.symmetric_fold_device(d_t.data_ptr(), words, 15, d_w.data_ptr(), half, folds.data_ptr())
    d_t2, d_w2 = to_device(tuples[half:]), to_device(weights[half:])
    native.symmetric_fold_device(d_t2.data_ptr(), words, 15, d_w2.data_ptr(), n - half,
                                 folds.data_ptr(), native.FLAG_ACCUMULATE)
    np.testing.assert_array_equal(folds.cpu().numpy().view(np.uint64), want)


@pytest.mark.parametrize("ipv6", [False, True])
@pytest.mark.parametrize("H,Q,kind,fields", [
    (128, 24, "none", 15), (1, 1, "none", 15), (100, 7, "none", 15), (16, 24, "none", 15),
    (65536, 24, "none", 15), (131072, 24, "none", 15), (100000, 45000, "none", 15),
    (128, 24, "max", 15), (128, 24, "random", 3),
    # byte lanes, 8 patterns per workgroup to Q = 79; half-word lanes, 4, lane-private to 159 ...
    (128, 79, "none", 15), (128, 80, "none", 15), (1024, 159, "none", 15), (1000, 159, "random", 15),
    # ... shared [pattern][queue] bins to 5088, then global atomics
    (1024, 160, "none", 15), (8192, 5088, "random", 15), (8192, 5089, "none", 15)])
def test_scan_matches_oracle(native, oracle_lib, H, Q, kind, fields, ipv6):
    from rss_simulator_nvidia_amd import keysearch
    n = 2003
    tuples = random_words(n, 9, H + Q) if ipv6 else oracle_lib.generate(H + Q, 0, n)
    weights = make_weights(kind, n, Q)
    for first, count in PATTERNS:
        loads = keysearch.symmetric_loads(tuples, H, Q, (first, count), ipv6, weights, fields)
        assert loads.shape == (count, min(H, Q)) and loads.dtype == np.uint64
        np.testing.assert_array_equal(
            loads, oracle_loads(oracle_lib, range(first, first + count), tuples, weights, H, Q, fields))


def test_full_range_is_exact_and_symmetric(native, oracle_lib):
    from rss_simulator_nvidia_amd import keysearch
    H, Q, n = 128, 24, 1 << 16
    tuples, weights = oracle_lib.generate(16, 0, n), make_weights("random", n, 1)
    loads = keysearch.symmetric_loads(tuples, H, Q, weights=weights)
    assert loads.shape == (65536, Q)
    assert (loads.sum(axis=1) == weights.sum(dtype=np.uint64)).all()
    sample = [0, 1, 0x6d5a, 0x8001, 0xFFFE, 0xFFFF]
    np.testing.assert_array_equal(loads[sample], oracle_loads(oracle_lib, sample, tuples, weights, H, Q))
    swapped = np.stack([tuples[:, 1], tuples[:, 0], (tuples[:, 2] << 16) | (tuples[:, 2] >> 16)], axis=1)
    np.testing.assert_array_equal(loads, keysearch.symmetric_loads(swapped, H, Q, weights=weights))


def test_graph_replay_follows_the_weights(native, oracle_lib):
    """The captured fold + scan clear their outputs themselves: each replay gives the loads of
    the weights then in the buffer, over whatever folds and loads held before."""
    n, H, Q, first, count = 4099, 128, 24, 0x6d58, 5
    host = oracle_lib.generate(21, 0, n)
    d_t, d_w = to_device(host), torch.zeros(n, dtype=torch.int32, device="cuda:0")
    folds = torch.empty(65536, dtype=torch.int64, device="cuda:0")
    loads = torch.empty((count, Q), dtype=torch.int64, device="cuda:0")

    def call():
        s = torch.cuda.current_stream().cuda_stream
        native.symmetric_fold_device(d_t.data_ptr(), 3, 15, d_w.data_ptr(), n, folds.data_ptr(), 0, s)
        native.symmetric_search_device(folds.data_ptr(), first, count, H, Q, loads.data_ptr(), s)

    call()  # eager first: code objects loaded before the capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for kind in ("random", "max", "random"):
        weights = make_weights(kind, n, 9)
        d_w.copy_(torch.from_numpy(weights.view(np.int32)))
        loads.fill_(3)
        folds.fill_(5)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(
            loads.cpu().numpy().view(np.uint64),
            oracle_loads(oracle_lib, range(first, first + count), host, weights, H, Q))


@pytest.mark.parametrize("source", ["csv", "pcap6"])
def test_cli_symmetric(native, oracle_lib, tmp_path, capsys, source):
    from rss_simulator_nvidia_amd import keysearch, pcap
    H, Q, rng = 128, 24, np.random.default_rng(8)
    if source == "csv":
        tuples = oracle_lib.generate(4, 0, 300)
        path = tmp_path / "flows.csv"
        path.write_text("src_ip,dst_ip,src_port,dst_port\n" + "".join(
            "%d.%d.%d.%d,%d.%d.%d.%d,%d,%d\n" % (*s.to_bytes(4, "big"), *d.to_bytes(4, "big"),
                                               p >> 16, p & 0xFFFF) for s, d, p in tuples.tolist()))
        argv, words, weights = ["--ips-file", str(path)], tuples, None
    else:
        flows = [pb.ether(pb.ipv6(rng.bytes(16), rng.bytes(16), 17,
                                  pb.l4(*(int(x) for x in rng.integers(1, 65536, 2)))), 0x86DD)
                 for _ in range(40)]
        path = tmp_path / "flows.pcap"
        path.write_bytes(pb.pcap_file([flows[f] for f in rng.integers(0, len(flows), 200)]))
        t6, _, _, weights = pcap.read_flows(str(path), ipv6=True, packet_counts=True)
        words = np.ascontiguousarray(t6).view(np.uint32).reshape(-1, 9)
        assert int(weights.sum()) == 200
        argv = ["--pcap", str(path), "--ipv6"]
    out = tmp_path / "best.txt"
    ranked = keysearch.main(argv + ["--symmetric", "--htable-size", str(H), "--num-queues", str(Q),
                                    "--top", "3", "--out", str(out)])
    lines = capsys.readouterr().out.splitlines()
    key = [int(x, 16) for x in out.read_text().split(":")]
    assert len(key) == 40 and key == key[:2] * 20 and lines[0].startswith(out.read_text())
    loads = oracle_loads(oracle_lib, [key[0] << 8 | key[1]], words, weights, H, Q)
    np.testing.assert_array_equal(loads[0], ranked[0]["counts"])
    printed = re.search(r"max_load (\S+)", lines[0]).group(1)
    assert printed == "%.4f" % keysearch.balance(loads, H, Q)["max_load"][0] and len(lines) == 3
