"""GPU parity for flow aggregation (rss_flow_aggregate_device / _host) against np.unique +
np.add.at in first-seen order: exact flows, loads, first and nflows."""
import numpy as np
import pytest

import pcap_builder as pb

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def native():
    from rss_simulator_nvidia_amd import _native
    if not torch.cuda.is_available():
        pytest.fail("gpu tests need a gfx950 device")
    return _native


def reference(tuples, weights):
    """(flows, loads, first) of (n, words) uint32 tuples by np.unique on the void view."""
    n, words = tuples.shape
    if n == 0:
        return tuples, np.zeros(0, np.uint64), np.zeros(0, np.uint32)
    raw = np.ascontiguousarray(tuples).view(np.dtype((np.void, 4 * words))).reshape(-1)
    _, first, inverse = np.unique(raw, return_index=True, return_inverse=True)
    loads = np.zeros(len(first), dtype=np.uint64)
    np.add.at(loads, inverse.reshape(-1),
              np.ones(n, np.uint64) if weights is None else weights.astype(np.uint64))
    order = np.argsort(first, kind="stable")
    return tuples[first[order]], loads[order], first[order].astype(np.uint32)


def random_words(n, words, seed):
    return np.random.default_rng(seed).integers(0, 2**32, (n, words), dtype=np.uint64).astype(np.uint32)


def make_case(name, words):
    """(tuples, weights) of the named input."""
    rng = np.random.default_rng(len(name) + words)
    if name.startswith("distinct"):
        n = int(name[8:])
        return random_words(n, words, n), None
    if name == "one_flow_max_weights":
        return np.repeat(random_words(1, words, 1), 4099, axis=0), np.full(4099, 0xFFFFFFFF, np.uint32)
    if name == "last_and_first_word":  # half differ from the base in the last word only, half in the first
        t = np.repeat(random_words(1, words, 2), 4099, axis=0)
        t[:2048, words - 1] = rng.integers(0, 600, 2048)
        t[2048:, 0] = rng.integers(0, 600, 2051)
        return t, rng.integers(0, 2**32, 4099, dtype=np.uint64).astype(np.uint32)
    if name == "mod997":
        return (random_words(997, words, 3)[np.arange(20011) % 997],
                rng.integers(0, 2**32, 20011, dtype=np.uint64).astype(np.uint32))
    assert name == "zipf"
    draws = (rng.zipf(1.2, (1 << 20) + 3) - 1) % 50000
    return random_words(50000, words, 4)[draws], None


CASES = ["distinct0", "distinct1", "distinct2", "distinct3", "distinct5", "one_flow_max_weights",
         "distinct4099", "last_and_first_word", "mod997", "zipf"]


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("words", [3, 9])
def test_matches_numpy(native, words, name):
    tuples, weights = make_case(name, words)
    flows, loads, first = native.default_context().aggregate_flows(tuples, weights, ipv6=words == 9)
    want_flows, want_loads, want_first = reference(tuples, weights)
    assert len(flows) == len(want_first)
    np.testing.assert_array_equal(first, want_first)
    np.testing.assert_array_equal(loads, want_loads)
    np.testing.assert_array_equal(flows, want_flows)
    assert flows.dtype == np.uint32 and loads.dtype == np.uint64 and first.dtype == np.uint32


def to_device(array, offset_words=0):
    """`array` on the GPU behind `offset_words` int32 of padding (a pointer = 4 mod 16 for 1)."""
    flat = torch.from_numpy(np.ascontiguousarray(array).view(np.int32).reshape(-1))
    buf = torch.empty(len(flat) + offset_words, dtype=torch.int32, device="cuda:0")
    buf[offset_words:] = flat.to("cuda:0")
    return buf[offset_words:]


@pytest.mark.parametrize("words", [3, 9])
def test_device_entry_misaligned_and_reused_workspace(native, words):
    """Tuples and weights at pointers = 4 mod 16 into garbage outputs; then a smaller, different
    input on the same workspace: nothing of the first call may show."""
    n = 20011
    ws_bytes = native.flow_aggregate_workspace_bytes(n, words)
    ws = torch.full((ws_bytes // 8,), 0x0101010101010101, dtype=torch.int64, device="cuda:0")
    flows = torch.full((n * words,), -1, dtype=torch.int32, device="cuda:0")
    loads = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
    first = torch.full((n,), -1, dtype=torch.int32, device="cuda:0")
    nflows = torch.full((1,), -1, dtype=torch.int64, device="cuda:0")
    for tuples, weights in (make_case("mod997", words), make_case("last_and_first_word", words)):
        m = len(tuples)
        d_t, d_w = to_device(tuples, 1), to_device(weights, 1)
        assert d_t.data_ptr() % 16 == 4 and d_w.data_ptr() % 16 == 4
        native.flow_aggregate_device(d_t.data_ptr(), words, d_w.data_ptr(), m, flows.data_ptr(),
                                     loads.data_ptr(), first.data_ptr(), nflows.data_ptr(),
                                     ws.data_ptr(), ws_bytes)
        want_flows, want_loads, want_first = reference(tuples, weights)
        f = int(nflows.cpu()[0])
        assert f == len(want_first)
        np.testing.assert_array_equal(first.cpu().numpy().view(np.uint32)[:f], want_first)
        np.testing.assert_array_equal(loads.cpu().numpy().view(np.uint64)[:f], want_loads)
        np.testing.assert_array_equal(
            flows.cpu().numpy().view(np.uint32)[:f * words].reshape(f, words), want_flows)


def test_cli_aggregate_and_pcap(native, oracle_lib, tmp_path, capsys):
    from rss_simulator_nvidia_amd import keysearch, pcap
    rng = np.random.default_rng(12)
    flow_set = oracle_lib.generate(9, 0, 60)
    packets = flow_set[rng.integers(0, 60, 500)]
    weights = rng.integers(1, 1500, 500)
    want_flows, want_loads, _ = reference(packets, weights.astype(np.uint32))

    def write(path, rows, column):
        path.write_text("src_ip,dst_ip,src_port,dst_port,bytes\n" + "".join(
            "%d.%d.%d.%d,%d.%d.%d.%d,%d,%d,%d\n" % (*s.to_bytes(4, "big"), *d.to_bytes(4, "big"),
                                                  p >> 16, p & 0xFFFF, w)
            for (s, d, p), w in zip(rows.tolist(), column.tolist())))
        return ["--ips-file", str(path), "--weight-column", "bytes", "--htable-size", "128",
                "--num-queues", "24", "--keys", "64", "--top", "3"]

    keysearch.main(write(tmp_path / "flows.csv", want_flows, want_loads))
    by_flow = capsys.readouterr().out
    keysearch.main(write(tmp_path / "packets.csv", packets, weights) + ["--aggregate"])
    assert capsys.readouterr().out == by_flow and len(by_flow.splitlines()) == 3

    frames = [pb.ether(pb.ipv4(bytes([10, 0, f, 1]), bytes([10, 1, 0, f]), 17, pb.l4(1000 + f, 53)))
              for f in range(30)]
    path = tmp_path / "repeats.pcap"
    path.write_bytes(pb.pcap_file([frames[f] for f in rng.integers(0, 30, 400)]))
    host = pcap.read_flows(str(path), packet_counts=True)
    device = pcap.read_flows(str(path), packet_counts=True, on_device=True)
    for a, b in zip(host, device):
        np.testing.assert_array_equal(a, b)
        assert np.asarray(a).dtype == np.asarray(b).dtype
