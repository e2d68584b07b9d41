"""GPU parity for flow aggregation (rss_flow_aggregate_device / _host) against np.unique +
np.add.at in first-seen order: exact flows, loads, first and nflows.  Random and heavy-tailed
inputs, and tuples with chosen hashes (flow_hash.preimage): probe chains that start on the last
slot of the combiner's local table and of the global one, wrap and run into each other.  Every
input goes through both insert kernels (RSS_AGGREGATE_COMBINER 1 and 0); one input is large
enough for the tile and chunk loops' further trips; one call is captured and replayed."""
import numpy as np
import pytest

import flow_hash as fh
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
    if name == "zipf":
        draws = (rng.zipf(1.2, (1 << 20) + 3) - 1) % 50000
        return random_words(50000, words, 4)[draws], None

    def u32(count):
        return rng.integers(0, 2**32, count, dtype=np.uint64).astype(np.uint32)

    def with_hashes(hashes):  # distinct flows (random but for the last word) with these hashes
        return fh.preimage(random_words(len(hashes), words - 1, len(name)), hashes)

    if name == "one_chain_repeated":  # duplicates atomicMin into a chain that is still growing
        flows = with_hashes(np.full(1500, 0xFFFFFFFF, np.uint32))
        packets = rng.permutation(np.repeat(np.arange(1500), rng.integers(2, 6, 1500)))
        return flows[packets], u32(len(packets))
    if name.startswith("one_chain"):  # one probe run from the last slot of both tables
        count = int(name[9:])
        return with_hashes(np.full(count, 0xFFFFFFFF, np.uint32)), u32(count)
    if name == "clusters_across_the_end":
        sizes, nslots = (400, 401, 399), 2 * fh.CHUNK[words]
        packets = rng.permutation(np.concatenate([np.arange(1200), rng.integers(0, 1200, 600)]))
        cap = fh.capacity(len(packets))
        starts = ((nslots - 2, cap - 3), (0, 0), (1, 1))  # (local, global) of the three groups
        flows = with_hashes(np.repeat([fh.hash_for_slots(l, g, words, cap) for l, g in starts], sizes))
        return flows[packets], u32(len(packets))
    if name == "local_only":  # the top 13 bits set: the last local slot, any global slot
        flows = with_hashes((0x1FFF << 19) | rng.choice(1 << 19, 2000, replace=False))
        return flows, u32(2000)
    if name == "global_only":  # the low 21 bits set: the last global slot, local slots all over
        flows = with_hashes((rng.permutation(2048)[:2000] << 21) | 0x1FFFFF)
        return flows, u32(2000)
    if name == "all_zero_weights":
        return random_words(997, words, 6)[np.arange(19940) % 997], np.zeros(19940, np.uint32)
    assert name == "ones_words"  # 0xFFFFFFFF is the tables' empty index, not an empty tuple
    rows = random_words(66, words, 7)
    rows[np.arange(64), np.arange(64) % words] = 0xFFFFFFFF
    rows[64], rows[65] = 0xFFFFFFFF, 0
    packets = rng.permutation(np.repeat(np.arange(66), 3))
    return rows[packets], u32(len(packets))


CASES = ["distinct0", "distinct1", "distinct2", "distinct3", "distinct5", "one_flow_max_weights",
         "distinct4099", "last_and_first_word", "mod997", "zipf"]
# forced collisions; table-size steps (2n == cap at 512 and 4096) and chunk edges; semantic edges
FORCED = ["one_chain512", "one_chain513", "one_chain4096", "one_chain4099", "one_chain_repeated",
          "clusters_across_the_end", "local_only", "global_only", "all_zero_weights", "ones_words",
          "distinct2047", "distinct2048", "distinct2049", "distinct3071", "distinct3072",
          "distinct3073"]


def test_forced_cases_are_what_they_claim():
    """The inputs' construction, by the numpy port: without it a changed hash would leave the
    cases below passing on what are then random tuples."""
    for words in (3, 9):
        nslots = 2 * fh.CHUNK[words]
        for name in ("one_chain4099", "one_chain_repeated"):
            tuples, _ = make_case(name, words)
            assert len(np.unique(tuples, axis=0)) == (4099 if name == "one_chain4099" else 1500)
            h = fh.agg_hash(tuples)
            assert (h == 0xFFFFFFFF).all() and fh.local_slot(h[0], words) == nslots - 1
        tuples, _ = make_case("clusters_across_the_end", words)
        h, cap = fh.agg_hash(tuples), fh.capacity(len(tuples))
        assert len(np.unique(tuples, axis=0)) == 1200
        assert sorted(set(zip(fh.local_slot(h, words).tolist(), (h & (cap - 1)).tolist()))) == [
            (0, 0), (1, 1), (nslots - 2, cap - 3)]
        h = fh.agg_hash(make_case("local_only", words)[0])
        assert (fh.local_slot(h, words) == nslots - 1).all() and len(set((h & 4095).tolist())) > 1000
        h = fh.agg_hash(make_case("global_only", words)[0])
        assert (h & 4095 == 4095).all() and len(set(fh.local_slot(h, words).tolist())) == 2000


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("words", [3, 9])
def test_matches_numpy(native, monkeypatch, words, name):
    monkeypatch.setenv("RSS_AGGREGATE_COMBINER", "1")
    tuples, weights = make_case(name, words)
    flows, loads, first = native.default_context().aggregate_flows(tuples, weights, ipv6=words == 9)
    want_flows, want_loads, want_first = reference(tuples, weights)
    assert len(flows) == len(want_first)
    np.testing.assert_array_equal(first, want_first)
    np.testing.assert_array_equal(loads, want_loads)
    np.testing.assert_array_equal(flows, want_flows)
    assert flows.dtype == np.uint32 and loads.dtype == np.uint64 and first.dtype == np.uint32


@pytest.mark.parametrize("combiner,name", [("0", name) for name in CASES + FORCED] +
                         [("1", name) for name in FORCED])
@pytest.mark.parametrize("words", [3, 9])
def test_both_insert_kernels(native, monkeypatch, words, combiner, name):
    """CASES through the direct insert kernel as well, FORCED through both."""
    monkeypatch.setenv("RSS_AGGREGATE_COMBINER", combiner)
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


class DeviceCall:
    """Outputs and workspace for n packets on the device entry, full of garbage until a call."""

    def __init__(self, native, n, words):
        self.native, self.n, self.words = native, n, words
        self.ws_bytes = native.flow_aggregate_workspace_bytes(n, words)
        self.ws = torch.empty(self.ws_bytes // 8, dtype=torch.int64, device="cuda:0")
        self.flows = torch.empty(n * words, dtype=torch.int32, device="cuda:0")
        self.loads = torch.empty(n, dtype=torch.int64, device="cuda:0")
        self.first = torch.empty(n, dtype=torch.int32, device="cuda:0")
        self.nflows = torch.empty(1, dtype=torch.int64, device="cuda:0")
        self.garbage()

    def garbage(self):
        self.ws.fill_(0x0101010101010101)
        for out in (self.flows, self.loads, self.first, self.nflows):
            out.fill_(-1)

    def __call__(self, d_tuples, d_weights, stream=None):
        self.native.flow_aggregate_device(
            d_tuples.data_ptr(), self.words, None if d_weights is None else d_weights.data_ptr(),
            self.n, self.flows.data_ptr(), self.loads.data_ptr(), self.first.data_ptr(),
            self.nflows.data_ptr(), self.ws.data_ptr(), self.ws_bytes, stream)

    def check(self, want):
        want_flows, want_loads, want_first = want
        f = int(self.nflows.cpu()[0])
        assert f == len(want_first)
        np.testing.assert_array_equal(self.first[:f].cpu().numpy().view(np.uint32), want_first)
        np.testing.assert_array_equal(self.loads[:f].cpu().numpy().view(np.uint64), want_loads)
        np.testing.assert_array_equal(
            self.flows[:f * self.words].cpu().numpy().view(np.uint32).reshape(f, self.words),
            want_flows)


@pytest.fixture(scope="module", params=[3, 9])
def many_tiles(request):
    """(words, tuples, weights, reference) of 3 * 2^20 + 1029 heavy-tailed packets: 3074 tiles
    (more than 8 workgroups per CU take in one trip, 4 tiles per lane of the scan with a ragged
    last lane), 1025 / 1537 chunks, and more than the direct kernel's grid holds at once."""
    words, n, rng = request.param, 3 * (1 << 20) + 1029, np.random.default_rng(request.param)
    tuples = random_words(200000, words, 5)[(rng.zipf(1.2, n) - 1) % 200000]
    weights = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return words, tuples, weights, reference(tuples, weights)


@pytest.mark.parametrize("combiner", ["1", "0"])
def test_many_tiles(native, monkeypatch, many_tiles, combiner):
    monkeypatch.setenv("RSS_AGGREGATE_COMBINER", combiner)
    words, tuples, weights, want = many_tiles
    d_t, d_w = to_device(tuples), to_device(weights)
    assert d_t.data_ptr() % 16 == 0 and d_w.data_ptr() % 16 == 0  # dwordx4 staging and groups
    run = DeviceCall(native, len(tuples), words)
    run(d_t, d_w)
    run.check(want)


@pytest.mark.parametrize("combiner", ["1", "0"])
@pytest.mark.parametrize("words", [3, 9])
def test_device_entry_without_weights(native, monkeypatch, words, combiner):
    """A NULL weights pointer on the device entry: loads are packet counts."""
    monkeypatch.setenv("RSS_AGGREGATE_COMBINER", combiner)
    tuples, _ = make_case("mod997", words)
    run = DeviceCall(native, len(tuples), words)
    run(to_device(tuples), None)
    run.check(reference(tuples, None))


@pytest.mark.parametrize("words", [3, 9])
def test_graph_replay_follows_the_buffers(native, monkeypatch, words):
    """One captured call, replayed over tuples and weights rewritten in place and over garbage in
    the outputs and the workspace: each replay is the aggregation of what the buffers hold then."""
    monkeypatch.setenv("RSS_AGGREGATE_COMBINER", "1")
    mod997 = make_case("mod997", words)
    n = len(mod997[0])
    chain, _ = make_case("one_chain_repeated", words)
    chain = (chain[np.arange(n) % len(chain)],
             np.random.default_rng(words).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32))
    d_t, d_w = to_device(mod997[0]), to_device(mod997[1])
    run = DeviceCall(native, n, words)

    def call():
        run(d_t, d_w, torch.cuda.current_stream().cuda_stream)

    call()  # eager first: code objects loaded before the capture
    run.check(reference(*mod997))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g):
            call()
    torch.cuda.current_stream().wait_stream(side)
    for tuples, weights in (mod997, chain, mod997):
        d_t.copy_(torch.from_numpy(tuples.view(np.int32).reshape(-1)))
        d_w.copy_(torch.from_numpy(weights.view(np.int32)))
        run.garbage()
        g.replay()
        torch.cuda.synchronize()
        run.check(reference(tuples, weights))


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
